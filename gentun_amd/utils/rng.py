"""Process-wide host RNG for the GA layer.

The reference draws every GA decision from the global ``random`` module and
never seeds it (gentun/individuals.py:10, gentun/algorithms.py:6; SURVEY.md
Q12). We keep one ``random.Random`` instance that starts OS-seeded (same
default behaviour) but can be seeded, snapshotted into a checkpoint and
restored, so a resumed or multi-GPU run replays the identical GA trajectory.

Device-side randomness (weight init, dropout, shuffles) never uses this
stream: it is keyed by (run seed, genes, fold, step) so fitness does not
depend on how candidates are spread over GPUs (SURVEY.md §7.3 hard part 4).
"""

import hashlib
import random

_RNG = random.Random()


def get():
    return _RNG


def seed(value):
    """Seed the GA stream (``None`` -> OS entropy, like the reference)."""
    _RNG.seed(value)


def get_state():
    """Serialisable snapshot of the GA stream (text, for JSON checkpoints)."""
    version, internal, gauss = _RNG.getstate()
    return {"version": version, "internal": list(internal), "gauss": gauss}


def set_state(state):
    _RNG.setstate((state["version"], tuple(state["internal"]), state["gauss"]))


def stable_hash(*parts):
    """64-bit hash that is identical on every rank / process / Python run
    (Python's ``hash`` of str is salted per process)."""
    h = hashlib.blake2b(digest_size=8)
    for p in parts:
        h.update(repr(p).encode())
        h.update(b"\x1f")
    return int.from_bytes(h.digest(), "little")



# ---------------------------------------------------------------------------
# numpy twins of the device hash (csrc/hip/common.h mix32 / hash4) and of the
# augmentation draw rule (csrc/hip/cnn_augment.hip): the torch executor and the
# test oracle draw through these, the HIP executor through the kernel
# ---------------------------------------------------------------------------

_M32 = 0xFFFFFFFF
AUG_CTR = 0xA0600000        # hash4 counters of the augmentation draws (no dense unit index reaches them)
FOLD_KEY_MUL = 0x632BE5AB   # fold id multiplier of the dropout / augmentation key


def _u32(x):
    import numpy as np
    return np.asarray(x).astype(np.uint64) & np.uint64(_M32)


def mix32(x):
    """common.h ``mix32`` on arrays of 32-bit values (held in uint64, wrapped to 32 bits)."""
    import numpy as np
    m = np.uint64(_M32)
    x = _u32(x)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    return x ^ (x >> np.uint64(16))


def hash4(a, b, c, d):
    """common.h ``hash4``; operands broadcast against each other. Returns uint64 arrays below 2**32."""
    import numpy as np
    m = np.uint64(_M32)
    h = mix32(_u32(a) ^ np.uint64(0x9E3779B9))
    h = mix32(h ^ _u32(b))
    h = mix32(h ^ ((_u32(c) * np.uint64(0x85EBCA6B)) & m))
    return mix32(h ^ ((_u32(d) * np.uint64(0xC2B2AE35)) & m))


def aug_key(seed, fold_id):
    """The per-group key of the dropout and augmentation streams: ``seed ^ (fold_id * 0x632be5ab)`` in 32 bits."""
    return (int(seed) ^ ((int(fold_id) * FOLD_KEY_MUL) & _M32)) & _M32


def aug_draws(key, step, rows, shift, flip):
    """``(dy, dx, flip)`` int64 arrays of the augmentation of batch rows ``rows`` (full-batch row numbers)
    at global step ``step`` under ``key`` (:func:`aug_key`); ``key`` / ``step`` / ``rows`` broadcast."""
    import numpy as np
    span = np.uint64(2 * int(shift) + 1)
    r0, r1, r2 = (hash4(key, step, rows, AUG_CTR + k) for k in range(3))
    dy = (r0 % span).astype(np.int64) - int(shift)
    dx = (r1 % span).astype(np.int64) - int(shift)
    fl = (r2 >> np.uint64(31)).astype(np.int64) if flip else np.zeros(r2.shape, np.int64)
    return dy, dx, fl
