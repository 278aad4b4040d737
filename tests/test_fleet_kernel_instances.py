"""CPU: each fleet kernel of csrc/fleet_kernels.hpp is instantiated in one form per translation unit -- the plain form (<false>) in
closed_loop.hip, observer.hip and race.hip, the delayed form (<true>) in actuator.hip, which holds launchers only.  With both forms of
a kernel in one translation unit LLVM allocates the plain form's registers differently (docs/HISTORY.md, "Fleet kernels as
templates")."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "autonomous-racing-lpv-mpp-mpc_amd", "csrc")
KERNELS = ("plant_kernel", "cl_measure_kernel", "cl_command_plant_measure_kernel", "cl_command_plant_observe_kernel",
           "race_measure_kernel", "race_command_plant_kernel", "race_command_plant_observe_kernel")


def source(fname):
    """The file without comments."""
    s = open(os.path.join(CSRC, fname)).read()
    return re.sub(r"//.*", "", re.sub(r"/\*.*?\*/", "", s, flags=re.S))


def instances(fname):
    """{(kernel, template argument)} of every fleet kernel named with a template argument list in the file."""
    return set(re.findall(r"\b(%s)\s*<\s*([^<>]*?)\s*>" % "|".join(KERNELS), source(fname)))


def test_plain_objects_instantiate_false_only():
    seen = set()
    for f in ("closed_loop.hip", "observer.hip", "race.hip"):
        inst = instances(f)
        assert inst and all(arg == "false" for _, arg in inst), (f, inst)
        seen |= {k for k, _ in inst}
    assert seen == set(KERNELS)


def test_actuator_instantiates_true_only_and_has_no_kernel_bodies():
    inst = instances("actuator.hip")
    assert inst == {(k, "true") for k in KERNELS}
    assert "__global__" not in source("actuator.hip")
