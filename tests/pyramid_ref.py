"""A plain numpy reference of the batched pyramid build (dvo_op_pyramid_frames), written from the contract text of include/dvo.h and
not from the kernels: the raw conversion, nearest-neighbour levels, the fused weight maps and a plan's copy-forward.

Everything is exact: integer arithmetic, single float32 multiplications and one float32 division per value, so the device is held to
it bit for bit (tests/test_gpu_pyramid_build.py).  tests/test_pyramid_ref.py pins it to the oracle without a GPU."""
import numpy as np

F32 = np.float32
INVALID = F32(-2.0)
SEQ_SKIP, SEQ_TRACK, SEQ_RESTART = 0, 1, 2
MAPS = ("gray", "depth", "sigma", "wgt")
UNWRITTEN = np.uint32(0xFFFFFFFF)   # what the op leaves in a map the build does not write


def luma(rgb):
    """u8 [..., 3 or 4] (R, G, B[, A]) -> the integer luma of dvo_op_ingest, as uint32"""
    r, g, b = (rgb[..., i].astype(np.uint32) for i in range(3))
    return (r * np.uint32(4899) + g * np.uint32(9617) + b * np.uint32(1868) + np.uint32(8192)) >> np.uint32(14)


def convert(rgb, depth16=None, depth_scale=0.0):
    """raw frames [n][rows][w] or [n][rows][w][3 or 4] (+ u16 depth) -> float32 (gray, depth, sigma); depth and sigma None without depth16"""
    rgb = np.asarray(rgb, np.uint8)
    g8 = rgb.astype(np.uint32) if rgb.ndim == 3 else luma(rgb)
    gray = g8.astype(F32) * F32(1.0 / 255.0)
    if depth16 is None:
        return gray, None, None
    d16 = np.asarray(depth16, np.uint16)
    scale = F32(depth_scale) if depth_scale > 0 else F32(1.0) / F32(5000.0)
    depth = d16.astype(F32) * scale
    sigma = np.where(d16 > 0, F32(0.1), F32(1.0)).astype(F32)
    gray = np.where(d16 == 0, INVALID, gray).astype(F32)
    return gray, depth, sigma


def pass_valid(a):
    """NaN and everything <= INVALID become INVALID; +inf stays"""
    a = np.asarray(a, F32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(a) | (a <= INVALID), INVALID, a).astype(F32)


def level_shape(w, h, levels, culls, l):
    t = levels - 1 - l
    return (h >> culls) >> t, (w >> culls) >> t


def level_of(src, w, h, levels, culls, l, row_shift=None):
    """level l of maps [n][rows][w].  row_shift: what the rows are already decimated by (None: whole frames)"""
    t = levels - 1 - l
    s = culls + t
    hl, wl = level_shape(w, h, levels, culls, l)
    ys = s if row_shift is None else s - row_shift
    sub = src[:, ::1 << ys, ::1 << s][:, :hl, :wl]
    if t == 0 and culls == 0:
        return np.ascontiguousarray(sub, F32).copy()   # the input unchanged
    return pass_valid(sub)


def steps(levels, step_default=2.0, step_level1=1.5, step_level2=1.0):
    return [F32(step_level1 if l == 1 else step_level2 if l == 2 else step_default) for l in range(levels)]


def weight(sigma, step, sigma_min=0.01, sigma_max=0.5):
    with np.errstate(invalid="ignore"):
        sc = np.minimum(np.maximum(np.asarray(sigma, F32), F32(sigma_min)), F32(sigma_max))
    return (F32(step) / sc).astype(F32)


def guards_fire(w, h, levels, culls):
    """(x, y): whether some level's lx >= w_l / ly >= h_l guard can fire, that is a kept top-level coordinate lands outside the level"""
    tw, th = w >> culls, h >> culls
    return (any(((tw - 1) >> t) >= (tw >> t) for t in range(levels)), any(((th - 1) >> t) >= (th >> t) for t in range(levels)))


def build(w, h, levels, culls, gray, depth=None, sigma=None, rows_decimated=False, cfg=None):
    """float maps [n][rows][w] (depth and sigma together or not at all) -> dict of per-level lists; maps the build does not write: None"""
    cfg = cfg or {}
    st = steps(levels, cfg.get("step_default", 2.0), cfg.get("step_level1", 1.5), cfg.get("step_level2", 1.0))
    rs = culls if rows_decimated else None
    out = {m: [None] * levels for m in MAPS}
    for l in range(levels):
        out["gray"][l] = level_of(gray, w, h, levels, culls, l, rs)
        if depth is not None:
            out["depth"][l] = level_of(depth, w, h, levels, culls, l, rs)
            out["sigma"][l] = level_of(sigma, w, h, levels, culls, l, rs)
            out["wgt"][l] = weight(out["sigma"][l], st[l], cfg.get("sigma_min", 0.01), cfg.get("sigma_max", 0.5))
    return out


def build_raw(w, h, levels, culls, rgb, depth16=None, depth_scale=0.0, rows_decimated=False, cfg=None):
    g, d, s = convert(rgb, depth16, depth_scale)
    return build(w, h, levels, culls, g, d, s, rows_decimated, cfg)


def planned(ref, new, actions, levels):
    """the set a planned build leaves: `new` (the build of the second frames) with every SKIP sequence replaced by `ref`'s top-level
    values decimated like a level (pass_valid below the top) and ref's wgt"""
    out = {m: [None if a is None else a.copy() for a in new[m]] for m in MAPS}
    T = levels - 1
    for q, act in enumerate(actions):
        if act != SEQ_SKIP:
            continue
        for l in range(levels):
            t = T - l
            for m in ("gray", "depth", "sigma"):
                if out[m][l] is None:
                    continue
                hl, wl = out[m][l].shape[1:]
                sub = ref[m][T][q, ::1 << t, ::1 << t][:hl, :wl]
                out[m][l][q] = sub if t == 0 else pass_valid(sub)
            if out["wgt"][l] is not None:
                out["wgt"][l][q] = ref["wgt"][l][q]
    return out
