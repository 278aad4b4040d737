"""The reference simulator's actuator model (vehicleSimulator.py:53-78) for the device fleets: motor / steering delays and the
low-level servo lag.  The device works in simulator steps; the reference is configured in seconds (simulator/delay_a,
simulator/delay_df) and builds its FIFOs with int(delay / dt).  These helpers make that conversion, truncation included."""
from __future__ import annotations

from . import _ffi


def delay_steps(delay_s, dt=0.005):
    """int(delay / dt), as vehicleSimulator.py:53-54 sizes a_his / df_his (int(0.145 / 0.005) = 28, not 29)."""
    return int(float(delay_s) / float(dt))


def actuator_config(delay_a_s=0.0, delay_df_s=0.0, low_level_dyn=False, dt_sim=0.005, servo_tf=0.07):
    """An ``_ffi.ActuatorConfig`` from the reference's launch parameters in seconds (simulator/delay_a, simulator/delay_df,
    simulator/lowLevelDyn, simulator/dt).  All off is the reference's launch file."""
    c = _ffi.ActuatorConfig()
    c.delay_a, c.delay_df = delay_steps(delay_a_s, dt_sim), delay_steps(delay_df_s, dt_sim)
    c.low_level_dyn = 1 if low_level_dyn else 0
    c.servo_tf = float(servo_tf)
    return c


def controller_delay(delay_df_s, dt=1.0 / 30.0):
    """Steering_Delay = int(delay_df / dt) (controllerMain.py:52): the controller's steeringDelay that matches a plant steering
    delay of delay_df_s seconds at the controller's rate."""
    return int(float(delay_df_s) / float(dt))
