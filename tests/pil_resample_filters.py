"""tests/pil_resample.py with the filter as a parameter: a numpy restatement of Pillow's resample of 8-bit-per-channel images (ImagingResample:
precompute_coeffs with the filter's function and support, normalize_coeffs_8bpc, the horizontal pass into a uint8 intermediate, then the vertical
pass; or the other order, which Image.resize picks for images more than 100 times taller than wide) for BILINEAR, BICUBIC and BOX.  The yardstick
of lpi_image_resample_u8_f; tests/test_image_filters_host.py pins it to Pillow itself.  Not a test module: a helper the tests import."""
import math

import numpy as np

from pil_resample import PRECISION_BITS, vertical_first

BILINEAR, BICUBIC, BOX = 2, 3, 4          # Pillow's Image.Resampling values = LPI_FILTER_*
NAMES = {"bilinear": BILINEAR, "bicubic": BICUBIC, "box": BOX}
SUPPORT = {BOX: 0.5, BILINEAR: 1.0, BICUBIC: 2.0}


def filter_fn(filter, x):
    """Pillow's filter function on a float64 array, in its association order."""
    if filter == BOX:
        return np.where((x > -0.5) & (x <= 0.5), 1.0, 0.0)
    x = np.abs(x)
    if filter == BILINEAR:
        return np.where(x < 1.0, 1.0 - x, 0.0)
    if filter == BICUBIC:
        a = -0.5
        inner = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        outer = (((x - 5) * x + 8) * x - 4) * a
        return np.where(x < 1.0, inner, np.where(x < 2.0, outer, 0.0))
    raise ValueError(f"filter {filter!r} is not restated here")


def coeffs(filter, in_size, out_size, first=0, count=None):
    """Fixed-point taps of output positions first .. first+count-1 of an in_size -> out_size resize: (xmin [count], k [count, ksize] int64, zero
    beyond each position's tap count)."""
    count = out_size - first if count is None else count
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = SUPPORT[filter] * filterscale
    ss = 1.0 / filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    xx = np.arange(first, first + count, dtype=np.float64)
    center = (xx + 0.5) * scale
    xmin = np.maximum(np.trunc((center - support) + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc((center + support) + 0.5).astype(np.int64), in_size) - xmin
    taps = np.arange(ksize, dtype=np.int64)[None, :]
    arg = (((taps + xmin[:, None]).astype(np.float64) - center[:, None]) + 0.5) * ss
    w = filter_fn(filter, arg)
    w = np.where(taps < xmax[:, None], w, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1]                      # sequential, in tap order
    k = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    kf = k * float(1 << PRECISION_BITS)
    ki = np.where(kf < 0, np.trunc(-0.5 + kf), np.trunc(0.5 + kf)).astype(np.int64)
    return xmin, ki


def _pass(filter, a, in_size, out_size, first, count, axis):
    """One separable pass over `axis` (0 rows, 1 columns) of an int array [H, W, 3] -> uint8 values (int64 array).  The sums are exact integers
    (int64); `assert` that they fit Pillow's int32 accumulator, which the kernel's 32-bit sums rely on as well."""
    xmin, k = coeffs(filter, in_size, out_size, first, count)
    acc = np.full(a.shape[:axis] + (count,) + a.shape[axis + 1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
    for t in range(k.shape[1]):
        idx = np.minimum(xmin + t, in_size - 1)
        kt = k[:, t]
        if not kt.any():
            continue
        if axis == 1:
            acc += a[:, idx, :] * kt[None, :, None]
        else:
            acc += a[idx, :, :] * kt[:, None, None]
    assert acc.size == 0 or (-(1 << 31) <= acc.min() and acc.max() < (1 << 31))
    return np.clip(acc >> PRECISION_BITS, 0, 255)


def resample_window(filter, src, out_w, out_h, ox=0, oy=0, sw=None, sh=None):
    """Window [ox, ox+sw) x [oy, oy+sh) of Image.fromarray(src).resize((out_w, out_h), filter), src HWC uint8 -> HWC uint8."""
    h, w = src.shape[:2]
    sw = out_w - ox if sw is None else sw
    sh = out_h - oy if sh is None else sh
    ymin, ky = coeffs(filter, h, out_h, oy, sh)
    lo = int(ymin.min())
    hi = int(min(h, ymin.max() + ky.shape[1]))
    rows = src[lo:hi].astype(np.int64)
    tmp = _pass(filter, rows, w, out_w, ox, sw, axis=1)           # the u8 intermediate of the rows the window needs
    acc = np.full((sh, sw, 3), 1 << (PRECISION_BITS - 1), dtype=np.int64)
    for t in range(ky.shape[1]):
        kt = ky[:, t]
        if not kt.any():
            continue
        idx = np.clip(np.minimum(ymin + t, h - 1) - lo, 0, tmp.shape[0] - 1)
        acc += tmp[idx, :, :] * kt[:, None, None]
    assert -(1 << 31) <= acc.min() and acc.max() < (1 << 31)
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resample_window_vfirst(filter, src, out_w, out_h, ox=0, oy=0, sw=None, sh=None):
    """resample_window in the vertical-first order: rows [oy, oy+sh) of the vertical pass over the whole width, rounded to uint8, then the
    horizontal pass of columns [ox, ox+sw)."""
    h, w = src.shape[:2]
    sw = out_w - ox if sw is None else sw
    sh = out_h - oy if sh is None else sh
    tmp = _pass(filter, src.astype(np.int64), h, out_h, oy, sh, axis=0)
    return _pass(filter, tmp, w, out_w, ox, sw, axis=1).astype(np.uint8)


def resize(filter, src, out_w, out_h):
    """Image.fromarray(src).resize((out_w, out_h), filter) for an HWC uint8 array."""
    if vertical_first(src.shape[1], src.shape[0], out_h):
        return resample_window_vfirst(filter, src, out_w, out_h)
    return resample_window(filter, src, out_w, out_h)


def apply(filter, src, desc, size):
    """A descriptor (x0, y0, x1, y1, rw, rh, ox, oy, flip) applied to an HWC uint8 image -> CHW uint8 [3, size, size] (what the 'u8' format gives)."""
    x0, y0, x1, y1, rw, rh, ox, oy, flip = (int(v) for v in desc)
    crop = np.ascontiguousarray(src[y0:y1, x0:x1])
    f = resample_window_vfirst if vertical_first(x1 - x0, y1 - y0, rh) else resample_window
    out = f(filter, crop, rw, rh, ox, oy, size, size)
    if flip:
        out = out[:, ::-1]
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def abs_tap_sums(filter, in_size, out_size):
    """sum |tap| of every output position of an in_size -> out_size resize (int64 [out_size]): 255 * that + 2^21 bounds every partial sum."""
    return np.abs(coeffs(filter, in_size, out_size)[1]).sum(axis=1)
