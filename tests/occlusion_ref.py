"""Plain per-pixel oracle of occlusion sensitivity (CnnClassifier.occlusion, csrc/hip/cnn_occlude.hip).

Written independently of the model code: explicit loops over cells and pixels, no slicing. The definition:

    a window starts every `stride` pixels from 0 and is `patch` pixels long; windows are added until one reaches
    the image's edge, and that last one is clipped to the image, not moved back into it
    cell (gi, gj) has the flat index gi * Gw + gj
    O_cell(img)[i, j, c] = fill[c] where row i lies in window gi and column j in window gj, else img[i, j, c]
"""

import numpy as np


def windows(size, patch, stride):
    """The ``(start, stop)`` pairs along one axis of ``size`` pixels, found by walking, not by the formula."""
    out, start = [], 0
    while True:
        out.append((start, min(start + patch, size)))
        if start + patch >= size:
            return out
        start += stride


def grid(H, W, patch, stride):
    return len(windows(H, patch, stride)), len(windows(W, patch, stride))


def occlude(img, cell, patch, stride, fill, stored_hw=None):
    """One image ``[Hr][Wr][C]`` with cell ``cell`` (flat index) replaced by ``fill`` (``C`` numbers), stored in
    ``stored_hw`` (zeros outside the real extent). ``cell=None``: the image as it is."""
    Hr, Wr, C = img.shape
    Hp, Wp = stored_hw or (Hr, Wr)
    rows, cols = windows(Hr, patch, stride), windows(Wr, patch, stride)
    out = np.zeros((Hp, Wp, C), img.dtype)
    if cell is not None:
        (y0, y1), (x0, x1) = rows[cell // len(cols)], cols[cell % len(cols)]
    for i in range(Hr):
        for j in range(Wr):
            for c in range(C):
                inside = cell is not None and y0 <= i < y1 and x0 <= j < x1
                out[i, j, c] = fill[c] if inside else img[i, j, c]
    return out


def views(x, patch, stride, fill):
    """``[n, Gh * Gw, H, W, C]``: every occluded copy of every image of ``x [n, H, W, C]``."""
    n, H, W, C = x.shape
    Gh, Gw = grid(H, W, patch, stride)
    f = np.broadcast_to(np.asarray(fill, x.dtype), (C,))
    return np.stack([np.stack([occlude(img, cell, patch, stride, f) for cell in range(Gh * Gw)]) for img in x])
