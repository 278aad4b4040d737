"""CPU: the delayed kernels of csrc/actuator.hip are copies of kernels of race.hip, closed_loop.hip and observer.hip (kept apart so
that the originals compile to the code they had).  Each copy must equal its original line for line, apart from the lines that make
it the delayed form: the actuator stage around plant_step and the u_old history step.  A fix made to one side only fails here."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "autonomous-racing-lpv-mpp-mpc_amd", "csrc")


def body(fname, kernel):
    """The statements of __global__ `kernel` (from its opening brace to the matching one), stripped, without comments."""
    s = open(os.path.join(CSRC, fname)).read()
    i = s.index(kernel + "(")
    i = s.index("{", i)
    depth, j = 0, i
    while True:
        if s[j] == "{":
            depth += 1
        elif s[j] == "}":
            depth -= 1
            if depth == 0:
                break
        j += 1
    lines = [re.sub(r"//.*", "", ln).strip() for ln in s[i + 1:j].splitlines()]
    return [ln for ln in lines if ln]


ACT = ("act_stage(", "a.k[b]", "a.La[b]", "a.servo[b]", "double ua, ud;", "plant_step(pc, st, ua, ud);", "uold_push(")


def core(lines, drop):
    return [ln.replace("act_plant_finite(", "plant_finite(") for ln in lines if not any(d in ln for d in drop)]


def test_race_measure_copy():
    orig = core(body("race.hip", "race_measure_kernel"), ("uo[b * 2 + 0] = r.cmd[b * 2 + 0]",))
    copy = core(body("actuator.hip", "race_measure_act_kernel"), ("uold_push(",))
    assert len(orig) > 50 and orig == copy


def test_race_command_plant_copies():
    for o, c in (("race_command_plant_kernel", "race_command_plant_act_kernel"),
                 ("race_command_plant_observe_kernel", "race_command_plant_observe_act_kernel")):
        orig = core(body("race.hip", o), ("plant_step(pc, st, motor, servo);", "for (int k = 0; k < n; ++k) {", "for (int k = 0; k < n; ++k) plant_step"))
        copy = core(body("actuator.hip", c), ACT + ("for (int k = 0; k < n; ++k) {",))
        orig = [ln for ln in orig if ln != "}"]; copy = [ln for ln in copy if ln != "}"]
        assert len(orig) > 15 and orig == copy, (o, [x for x in orig if x not in copy], [x for x in copy if x not in orig])


def test_cl_command_plant_measure_copy():
    orig = core(body("closed_loop.hip", "cl_command_plant_measure_kernel"),
                ("plant_step(pc, st, motor, servo);", "u_old[b * 2 + 0] = servo", "double s, ey, epsi; int inside;", "local_position(",
                 "double *ls = local_next", "ls[0] =", "ls[3] ="))
    copy = core(body("actuator.hip", "cl_command_plant_measure_act_kernel"), ACT + ("for (int k = 0; k < pc.n_sub; ++k) {", "cl_local("))
    orig = [ln for ln in orig if ln != "}"]; copy = [ln for ln in copy if ln != "}"]
    assert len(orig) > 8 and orig == copy, ([x for x in orig if x not in copy], [x for x in copy if x not in orig])
