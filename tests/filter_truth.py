"""numpy restatement of the edge-preserving depth filter (include/youth_filter.h,
DESIGN.md §11), written from the definition, not from the kernel: the truth of
test_filter.py and test_gpu_filter.py.

All integer.  For a pixel with centre c > 0 the gate is
T = min(255, t0 + ((t2 * (c >> 4)^2) >> 16)); a tap of the 5x5 window
contributes iff it is inside the frame, its depth n is > 0 and |n - c| < T,
with weight (T^2 - (n - c)^2) * ws[dy + 2] * ws[dx + 2], ws = {1, 2, 4, 2, 1};
out = c - T + floor((num + (den >> 1)) / den) with den = sum w and
num = sum w * (n - c + T).  A centre <= 0 is copied."""
import numpy as np

WS = (1, 2, 4, 2, 1)
DEFAULT_T0, DEFAULT_T2 = 8, 96


def gate(c, t0, t2):
    """T of centre depths c (> 0), int64."""
    c = np.asarray(c, np.int64)
    return np.minimum(255, t0 + ((t2 * (c >> 4) ** 2) >> 16))


def filter_truth(depth, t0=DEFAULT_T0, t2=DEFAULT_T2):
    """depth int16 [H][W] or [n][H][W] -> the filtered frame(s), int16."""
    d = np.asarray(depth)
    assert d.dtype == np.int16 and d.ndim in (2, 3)
    assert 1 <= t0 <= 255 and 0 <= t2 <= 1000
    if d.ndim == 3:
        return np.stack([filter_truth(f, t0, t2) for f in d]) if d.shape[0] else d.copy()
    H, W = d.shape
    c = d.astype(np.int64)
    valid = c > 0
    T = gate(np.where(valid, c, 1), t0, t2)
    pad = np.zeros((H + 4, W + 4), np.int64)      # out of frame: 0, never contributes
    pad[2:H + 2, 2:W + 2] = c
    num = np.zeros((H, W), np.int64)
    den = np.zeros((H, W), np.int64)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            n = pad[2 + dy:2 + dy + H, 2 + dx:2 + dx + W]
            delta = n - c
            on = (n > 0) & (np.abs(delta) < T)
            w = np.where(on, (T * T - delta * delta) * (WS[dy + 2] * WS[dx + 2]), 0)
            den += w
            num += w * (delta + T)
    assert int(num.max(initial=0)) < 2 ** 32 and int(den.max(initial=0)) < 2 ** 25
    den = np.where(valid, den, 1)
    out = c - T + (num + (den >> 1)) // den
    out = np.where(valid, out, c)
    assert np.array_equal(out > 0, valid)
    return out.astype(np.int16)
