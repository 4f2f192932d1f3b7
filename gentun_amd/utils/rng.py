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


MIX_CTR = 0xA0610000        # hash4 counters of the mixup / cutmix draws (models/cnn_engine.py "The mixed step")
MIX_KINDS = {"mixup": 0, "cutmix": 1}
MIX_MAX_ALPHA = 8
_ONE24 = 1 << 24


def mix_p24(prob):
    """``round(prob * 2^24)``: a step is mixed iff its 24-bit draw is below this."""
    return int(round(float(prob) * _ONE24))


def mix_box(cy, cx, m, hr, wr):
    """``(y0, y1, x0, x1)`` of the cutmix box centred at ``(cy, cx)`` under the 24-bit draw ``m``: sides
    ``isqrt((Hr Hr (2^24 - m)) >> 24)`` and likewise for ``Wr``, clipped to the image. Python integers."""
    import math
    cy, cx, m, hr, wr = int(cy), int(cx), int(m), int(hr), int(wr)
    bh = math.isqrt((hr * hr * (_ONE24 - m)) >> 24)
    bw = math.isqrt((wr * wr * (_ONE24 - m)) >> 24)
    ty, tx = cy - bh // 2, cx - bw // 2
    return max(ty, 0), min(ty + bh, hr), max(tx, 0), min(tx + bw, wr)


def mix_weights(kind, m, box, hr, wr):
    """``(lam, lam1)`` as numpy fp32: the weights of a row and of its partner in the mixed target (and, for
    mixup, in the mixed image). mixup: ``m 2^-24`` and ``(2^24 - m) 2^-24``, both exact; cutmix: the kept and
    the pasted share of the area, ``fp32(Hr Wr - area) * inv_hw`` and ``fp32(area) * inv_hw`` with
    ``inv_hw = fp32(1) / fp32(Hr Wr)``."""
    import numpy as np
    if kind == "mixup":
        s = np.float32(2.0 ** -24)
        return np.float32(int(m)) * s, np.float32(_ONE24 - int(m)) * s
    y0, y1, x0, x1 = box
    area, hw = (y1 - y0) * (x1 - x0), int(hr) * int(wr)
    inv_hw = np.float32(np.float32(1.0) / np.float32(hw))
    return np.float32(np.float32(hw - area) * inv_hw), np.float32(np.float32(area) * inv_hw)


def mix_draws(key, step, nv, alpha, p24, hw):
    """The mixup / cutmix draw of global step ``step`` under ``key`` (:func:`aug_key`) for batches of ``nv``
    real rows; ``key`` / ``step`` / ``nv`` broadcast. Returns int64 arrays ``(applied, o, m, cy, cx)``:
    whether the step is mixed, the partner offset (``p(b) = (b + o) % nv``), the 24-bit median of
    ``2 alpha - 1`` uniforms (Beta(alpha, alpha) * 2^24) and the cutmix centre in the real image ``hw``.
    ``o`` and ``m`` are 0 where the step is not mixed."""
    import numpy as np
    key, step, nv = np.broadcast_arrays(_u32(key), _u32(step), np.asarray(nv, np.int64))
    r = [hash4(key, step, 0, MIX_CTR + k) for k in range(4)]
    applied = (nv >= 2) & ((r[0] >> np.uint64(8)) < np.uint64(int(p24)))
    o = np.where(applied, 1 + (r[1] % np.maximum(nv - 1, 1).astype(np.uint64)).astype(np.int64), 0)
    u = np.stack([hash4(key, step, 0, MIX_CTR + 16 + j) >> np.uint64(8) for j in range(2 * int(alpha) - 1)])
    m = np.where(applied, np.sort(u, axis=0)[int(alpha) - 1].astype(np.int64), 0)
    cy = (r[2] % np.uint64(int(hw[0]))).astype(np.int64)
    cx = (r[3] % np.uint64(int(hw[1]))).astype(np.int64)
    return applied.astype(np.int64), o, m, cy, cx


MC_KEY = 0x4D434452        # hash4 counter of the Monte-Carlo dropout member key ("MCDR")


def mc_threshold(dropout):
    """``uint32(dropout * 2^32)``: a unit is kept iff its draw is at least this (``dense_fwd_epilogue``'s rule)."""
    return int(float(dropout) * 4294967296.0) & _M32


def mc_masks(seed, member, samples, rows, units, dropout):
    """Keep masks of Monte-Carlo dropout (csrc/hip/cnn_head_mc.hip), bool ``[samples, len(rows), units]``:
    sample ``t``, image index ``n = rows[i]`` and unit ``u`` are kept iff
    ``hash4(hash4(seed, member, MC_KEY, 0), t, n, u) >= mc_threshold(dropout)``."""
    import numpy as np
    key = hash4(int(seed), int(member), MC_KEY, 0)
    t = np.arange(int(samples), dtype=np.uint64)[:, None, None]
    n = np.asarray(rows, dtype=np.uint64).reshape(1, -1, 1)
    u = np.arange(int(units), dtype=np.uint64)[None, None, :]
    return hash4(key, t, n, u) >= np.uint64(mc_threshold(dropout))


SG_KEY = 0x534D4752        # xor of the seed in the key of the SmoothGrad noise draws ("SMGR")


def sg_noise(seed, n, samples, hr, wr, cr):
    """Standard normal draws of ``saliency(smooth=...)`` (csrc/hip/cnn_smooth.hip), fp64
    ``[len(n), samples, hr, wr, cr]``: for image index ``n`` (its index within the call; an integer or an array
    of them), sample ``k``, pixel ``p = i * wr + j`` and channel ``c``, Box-Muller's cosine branch
    ``z = sqrt(-2 ln u_0) * cos(2 pi u_1)`` of ``u_j = ((r_j >> 9) * 2 + 1) * 2^-24`` with
    ``r_j = hash4(seed ^ SG_KEY, n, k, (p * 4 + c) * 2 + j)``. ``u_j`` lies in (0, 1), so ``|z| <= 5.77``.
    ``samples`` is the number of samples (``k = 0 .. samples - 1``) or a sequence of sample indices ``k``."""
    import numpy as np
    key = (int(seed) ^ SG_KEY) & _M32
    nn = np.atleast_1d(np.asarray(n)).astype(np.uint64).reshape(-1, 1, 1, 1)
    k = np.arange(samples) if np.ndim(samples) == 0 else np.asarray(samples)
    k = k.astype(np.uint64).reshape(1, -1, 1, 1)
    p = np.arange(int(hr) * int(wr), dtype=np.uint64).reshape(1, 1, -1, 1)
    c = np.arange(int(cr), dtype=np.uint64).reshape(1, 1, 1, -1)
    d = (p * np.uint64(4) + c) * np.uint64(2)
    u = [((hash4(key, nn, k, d + np.uint64(j)) >> np.uint64(9)) * np.uint64(2) + np.uint64(1)).astype(np.float64)
         * 2.0 ** -24 for j in range(2)]
    z = np.sqrt(-2.0 * np.log(u[0])) * np.cos(2.0 * np.pi * u[1])
    return z.reshape(nn.shape[0], k.shape[1], int(hr), int(wr), int(cr))
