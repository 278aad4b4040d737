"""Race snapshots on the host (include/lpvmpc.h, "Race snapshot, restore and clone"): the blob that lpvmpc_race_snapshot writes and
lpvmpc_race_restore reads, parsed and rebuilt with ``struct`` and numpy alone -- no library, no device -- plus the host definition of
lpvmpc_race_clone on a blob (``take``) and the choice of sources of ``RaceFleet.respawn`` (``respawn_sources``).

Blob, version 1, little-endian: a 64 B header (magic "LPVRACE\\0"; int32 version, B, N, Np, M, sd, lap_cols, laps, ticks, features,
count, 3 x 0), ``count`` directory entries of 40 B (name[16], int32 type, W, layout, 0, int64 offset) and the arrays as they lie on
the device, each on a multiple of 8 B."""
import struct
from collections import OrderedDict

import numpy as np

MAGIC = b"LPVRACE\0"
VERSION = 1
HEADER_BYTES = 64
ENTRY_BYTES = 40
F64, I32 = 0, 1                               # LPVMPC_SNAP_F64 / _I32
VEHICLE_MAJOR, WORD_MAJOR = 0, 1              # [B][W] / [W][B]
HAS_ESTIMATOR, HAS_ACTUATOR, HAS_DISTURBANCES, HAS_TRACKS = 1, 2, 4, 8
HAS_TYRE_WEAR = 16                            # the arrays "wear.state" [B, 6] and "wear.rows" [B, 12] (tyre_wear.py) are carried
WEAR_ARRAYS = ("wear.state", "wear.rows")
HEADER_FIELDS = ("version", "B", "N", "Np", "M", "sd", "lap_cols", "laps", "ticks", "features", "count")
_HEADER = struct.Struct("<8s11i12x")
_ENTRY = struct.Struct("<16s4iq")
_DTYPES = {F64: np.dtype("<f8"), I32: np.dtype("<i4")}
assert _HEADER.size == HEADER_BYTES and _ENTRY.size == ENTRY_BYTES


def _align8(n):
    return (n + 7) & ~7


class RaceSnapshot(object):
    """One race snapshot.  ``header``: dict of HEADER_FIELDS; ``arrays``: OrderedDict name -> array normalised to vehicle-major
    [B, W] (word-major device arrays are transposed here and back in ``to_bytes``); ``directory``: name -> (type, W, layout), in
    the blob's order."""

    def __init__(self, header, directory, arrays):
        self.header = dict(header)
        self.directory = OrderedDict(directory)
        self.arrays = OrderedDict(arrays)

    @property
    def B(self):
        return self.header["B"]

    @property
    def ticks(self):
        return self.header["ticks"]

    @classmethod
    def from_bytes(cls, blob):
        blob = bytes(blob)
        if len(blob) < HEADER_BYTES:
            raise ValueError("race snapshot: %d B is shorter than the %d B header" % (len(blob), HEADER_BYTES))
        f = _HEADER.unpack_from(blob, 0)
        if f[0] != MAGIC:
            raise ValueError("race snapshot: wrong magic %r" % (f[0],))
        header = dict(zip(HEADER_FIELDS, f[1:]))
        if header["version"] != VERSION:
            raise ValueError("race snapshot: format version %d, this reader knows version %d" % (header["version"], VERSION))
        B, count = header["B"], header["count"]
        if B <= 0 or count < 0 or HEADER_BYTES + ENTRY_BYTES * count > len(blob):
            raise ValueError("race snapshot: truncated directory (B=%d, %d arrays, %d B)" % (B, count, len(blob)))
        directory, arrays = OrderedDict(), OrderedDict()
        for i in range(count):
            name, typ, W, layout, _, off = _ENTRY.unpack_from(blob, HEADER_BYTES + ENTRY_BYTES * i)
            name = name.rstrip(b"\0").decode("ascii")
            if typ not in _DTYPES or layout not in (VEHICLE_MAJOR, WORD_MAJOR) or W <= 0 or name in directory:
                raise ValueError("race snapshot: bad directory entry %d (%r: type %d, W %d, layout %d)" % (i, name, typ, W, layout))
            dt = _DTYPES[typ]
            n = B * W * dt.itemsize
            if off < 0 or off % 8 or off + n > len(blob):
                raise ValueError("race snapshot: truncated: array %r needs bytes %d .. %d of %d" % (name, off, off + n, len(blob)))
            a = np.frombuffer(blob, dt, B * W, off)
            a = a.reshape(W, B).T if layout == WORD_MAJOR else a.reshape(B, W)
            directory[name] = (typ, W, layout)
            arrays[name] = np.array(a, order="C")
        return cls(header, directory, arrays)

    def to_bytes(self):
        names = list(self.directory)
        at = HEADER_BYTES + ENTRY_BYTES * len(names)
        head, body = [], []
        for name in names:
            typ, W, layout = self.directory[name]
            a = np.asarray(self.arrays[name], _DTYPES[typ]).reshape(self.B, W)
            raw = (a.T if layout == WORD_MAJOR else a).tobytes(order="C")
            head.append(_ENTRY.pack(name.encode("ascii"), typ, W, layout, 0, at))
            body.append(raw + b"\0" * (_align8(len(raw)) - len(raw)))
            at += len(body[-1])
        h = dict(self.header, count=len(names))
        return _HEADER.pack(MAGIC, *[int(h[k]) for k in HEADER_FIELDS]) + b"".join(head) + b"".join(body)

    def take(self, src):
        """The host definition of lpvmpc_race_clone: a snapshot in which vehicle b holds every state word of vehicle src[b]."""
        src = np.asarray(src, np.int64).reshape(-1)
        if src.shape[0] != self.B or (src < 0).any() or (src >= self.B).any():
            raise ValueError("take: src must be [B] indices in [0, %d)" % self.B)
        return RaceSnapshot(self.header, self.directory, OrderedDict((k, np.ascontiguousarray(v[src])) for k, v in self.arrays.items()))

    def save(self, file):
        """Write an .npz: the header fields, the directory and the arrays (vehicle-major)."""
        names = list(self.directory)
        out = {"header": np.array([int(self.header[k]) for k in HEADER_FIELDS], np.int64), "names": np.array(names),
               "directory": np.array([self.directory[k] for k in names], np.int64).reshape(len(names), 3)}
        for k in names:
            out["array." + k] = self.arrays[k]
        np.savez(file, **out)

    @classmethod
    def load(cls, file):
        with np.load(file, allow_pickle=False) as z:
            header = dict(zip(HEADER_FIELDS, (int(v) for v in z["header"])))
            names = [str(n) for n in z["names"]]
            directory = OrderedDict((n, tuple(int(v) for v in row)) for n, row in zip(names, z["directory"]))
            arrays = OrderedDict((n, np.array(z["array." + n])) for n in names)
        return cls(header, directory, arrays)


def respawn_sources(alive, track_of, seed, lost=None):
    """The ``src`` map of ``RaceFleet.respawn``: every lost slot takes an alive vehicle of its own track, drawn uniformly by
    ``numpy.random.default_rng(seed)``; every other slot maps to itself.  ``alive`` [B] bool: vehicles that are still driving (the
    possible sources); ``lost`` [B] bool: the slots to fill (default: ``~alive``; a finished vehicle is neither -- it is frozen, not
    lost); ``track_of`` [B] or None (one track).  A track with no alive vehicle leaves its lost slots alone."""
    alive = np.asarray(alive, bool).reshape(-1)
    B = alive.shape[0]
    lost = ~alive if lost is None else np.asarray(lost, bool).reshape(-1)
    of = np.zeros(B, np.int64) if track_of is None else np.asarray(track_of, np.int64).reshape(-1)
    if lost.shape[0] != B or of.shape[0] != B:
        raise ValueError("respawn_sources: alive, lost and track_of must have one entry per vehicle")
    if (alive & lost).any():
        raise ValueError("respawn_sources: a vehicle is both alive and lost")
    rng = np.random.default_rng(seed)
    src = np.arange(B, dtype=np.int32)
    for t in np.unique(of):                                # ascending: the draws are a function of (alive, lost, track_of, seed)
        pool = np.flatnonzero(alive & (of == t))
        slots = np.flatnonzero(lost & (of == t))
        if pool.size and slots.size:
            src[slots] = pool[rng.integers(0, pool.size, slots.size)]
    return src
