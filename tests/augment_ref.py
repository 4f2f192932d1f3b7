"""Plain numpy oracle of the shift-and-flip training augmentation (TrainConfig.augment).

Written independently of the executors: explicit loops over rows and pixels, Python integers for the
hash. The definition (csrc/hip/cnn_augment.hip, gentun_amd/utils/rng.aug_draws):

    key  = seed ^ (fold_id * 0x632be5ab)                       (32 bits)
    r_k  = hash4(key, step, row, 0xA0600000 + k),  k = 0, 1, 2
    dy   = r_0 % (2 s + 1) - s,  dx = r_1 % (2 s + 1) - s,  flip = flip_enabled and (r_2 >> 31)
    out[i, j, c] = src[i - dy, f(j - dx), c] inside the real extent, else 0;  f(u) = Wr - 1 - u if flip else u
"""

import numpy as np

M = 0xFFFFFFFF


def mix32(x):
    x &= M
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M
    x ^= x >> 15
    x = (x * 0x846CA68B) & M
    x ^= x >> 16
    return x


def hash4(a, b, c, d):
    h = mix32((a & M) ^ 0x9E3779B9)
    h = mix32(h ^ (b & M))
    h = mix32(h ^ (((c & M) * 0x85EBCA6B) & M))
    return mix32(h ^ (((d & M) * 0xC2B2AE35) & M))


def key_of(seed, fold_id):
    return ((seed & M) ^ ((fold_id * 0x632BE5AB) & M)) & M


def draw(key, step, row, shift, flip):
    """(dy, dx, flip) of one batch row."""
    r = [hash4(key, step, row, 0xA0600000 + k) for k in range(3)]
    span = 2 * shift + 1
    return r[0] % span - shift, r[1] % span - shift, int(bool(flip) and (r[2] >> 31) == 1)


def transform(img, dy, dx, flip, stored_hw=None):
    """One image ``[Hr][Wr][C]`` under (dy, dx, flip), stored in ``stored_hw`` (zeros outside the real extent)."""
    Hr, Wr, C = img.shape
    Hp, Wp = stored_hw or (Hr, Wr)
    out = np.zeros((Hp, Wp, C), img.dtype)
    for i in range(Hr):
        for j in range(Wr):
            si, u = i - dy, j - dx
            if 0 <= si < Hr and 0 <= u < Wr:
                out[i, j] = img[si, Wr - 1 - u if flip else u]
    return out


def augment_batch(data, ids, seeds, fold_ids, step, shift, flip, real_hw, stored_hw=None, stored_c=None, row_off=0):
    """The stored-layout augmented batch ``[G][B][Hp][Wp][Cp]``.

    ``data``: the dataset in NHWC (the first ``real_hw`` rows / columns of every image are the real extent);
    ``ids [G][B]``: sample ids; ``seeds [G]`` / ``fold_ids [G]``: key material per group; ``step``: the global
    step; ``row_off``: the full-batch row of column 0 of ``ids`` (data parallelism)."""
    Hr, Wr = real_hw
    Hp, Wp = stored_hw or (Hr, Wr)
    C = data.shape[-1]
    Cp = stored_c or C
    ids = np.asarray(ids)
    G, B = ids.shape
    out = np.zeros((G, B, Hp, Wp, Cp), data.dtype)
    for g in range(G):
        key = key_of(int(seeds[g]), int(fold_ids[g]))
        for b in range(B):
            dy, dx, fl = draw(key, int(step), b + row_off, shift, flip)
            out[g, b, :, :, :C] = transform(data[int(ids[g, b]), :Hr, :Wr], dy, dx, fl, (Hp, Wp))
    return out
