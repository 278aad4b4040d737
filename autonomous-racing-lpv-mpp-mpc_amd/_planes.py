"""The planes of a race attachment (heats, interactions, contact model, walls, event log), [W, B] each, on the host: the named view of the output
planes and the carried state "just attached"."""
from __future__ import annotations

import numpy as np


def planes_dict(f, i, f_names, i_names):
    """Output planes f [len(f_names), B], i [len(i_names), B] -> dict of [B] arrays under those names and the planes themselves (f64,
    i32)."""
    out = {k: f[c] for c, k in enumerate(f_names)}
    out.update({k: i[c] for c, k in enumerate(i_names)})
    out.update(f64=f, i32=i)
    return out


def blank_carry(B, wf, carry_i_names, minus_one=()):
    """A carried state of zeros, f64 [wf, B] / i32 [len(carry_i_names), B], with the i32 words named in ``minus_one`` set to -1."""
    c = dict(f64=np.zeros((wf, B)), i32=np.zeros((len(carry_i_names), B), np.int32))
    for k in minus_one:
        c["i32"][carry_i_names.index(k)] = -1
    return c
