"""Numpy replica of the photometric calibration fused into the mono ingest (dvo_batch_set_photometric), the
calibrations the tests share, and a camera simulator.

    gray = inv_response[g8] * (1.0f / vignette[p])      float32: one division, one multiply
    gray = INVALID (-2)                                  where vignette[p] is not finite or <= 0

g8 is the byte of a 1-channel frame or lockstep.raw_gray's fixed-point luma of a colour frame (the response is applied to the
luma, not per channel)."""
import numpy as np

INVALID = np.float32(-2.0)
MASKED = np.float32(-1.0)   # the gain table's entry of a masked pixel / of the remap's border


def identity_response():
    """(float)i * (float)(1.0 / 255.0): k_ingest's scale, what a NULL inv_response means"""
    return np.arange(256, dtype=np.float32) * np.float32(1.0 / 255.0)


def luma_u8(frame_u8):
    """the byte the response is looked up with: the frame itself (1 channel) or k_ingest's fixed-point luma (3 / 4 channels)"""
    from real_data import bgr2gray_u8
    a = np.asarray(frame_u8, np.uint8)
    return a if a.ndim == 2 else bgr2gray_u8(a)


def gain_np(V, shape):
    """float32 `shape`: 1 / V, MASKED where V is not finite or <= 0; V None: ones"""
    if V is None:
        return np.ones(shape, np.float32)
    V = np.asarray(V, np.float32)
    ok = np.isfinite(V) & (V > 0)
    with np.errstate(divide="ignore", over="ignore"):
        return np.where(ok, np.float32(1.0) / np.where(ok, V, np.float32(1.0)), MASKED).astype(np.float32)


def correct_np(u8, lut=None, V=None):
    """The full-resolution float frame the library's pixels come from: lut[luma] * (1 / V), INVALID where V masks the pixel."""
    g8 = luma_u8(u8)
    lut = identity_response() if lut is None else np.asarray(lut, np.float32)
    g = gain_np(V, g8.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        out = lut[g8] * g                     # float32 * float32: one rounding
    return np.where(g < 0, INVALID, out).astype(np.float32)


def gain_table_np(V, w, h, K=None, D=None):
    """The gain table a sequence reads, float32 [h/4, w/4]: gain_np(V) at each kept pixel's source -- (x << 2, y << 2), or with a lens
    (K, D) the source index of real_data.undistort_index_np, whose -1 (the border) gives MASKED."""
    g = gain_np(V, (h, w))
    if D is None:
        return np.ascontiguousarray(g[0:(h // 4) * 4:4, 0:(w // 4) * 4:4])
    from real_data import undistort_index_np
    idx = undistort_index_np(K, D, w, h)[0:(h // 4) * 4:4, 0:(w // 4) * 4:4]
    out = np.full(idx.shape, MASKED, np.float32)
    out[idx >= 0] = g.reshape(-1)[idx[idx >= 0]]
    return out


# ---------------------------------------------------------------- the calibrations of the tests
def gamma_response(gamma=2.2):
    """inverse of a gamma curve: the sensor wrote u8 = 255 * irradiance ** (1 / gamma)"""
    return (np.arange(256, dtype=np.float64) / 255.0) ** gamma


def gamma_forward(gamma=2.2):
    """the forward response of gamma_response for expose(): irradiance in [0, 1] -> u8 value in [0, 255]"""
    return lambda e: 255.0 * np.clip(e, 0.0, 1.0) ** (1.0 / gamma)


def s_curve_response():
    """a measured-looking inverse response: monotone, a toe and a shoulder, 0 -> 0 and 255 -> 1"""
    x = np.arange(256, dtype=np.float64) / 255.0
    s = 0.5 - 0.5 * np.cos(np.pi * x)         # smoothstep-like S
    return 0.35 * x + 0.65 * s ** 1.3


def cos4_vignette(w, h, corner=0.4, cx=None, cy=None):
    """cos^4 fall-off that reaches `corner` at the image corner farthest from the centre (cx, cy)"""
    cx = (w - 1) / 2.0 if cx is None else cx
    cy = (h - 1) / 2.0 if cy is None else cy
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    r2 = (x - cx) ** 2 + (y - cy) ** 2
    f2 = r2.max() / (corner ** -0.5 - 1.0)    # cos^4(theta) = (1 + r^2 / f^2)^-2 = corner at the farthest corner
    return ((1.0 + r2 / f2) ** -2).astype(np.float32)


def masked_vignette(w, h):
    """an off-centre vignette with a masked bottom band (a bonnet): zeros in the last tenth of the rows"""
    V = cos4_vignette(w, h, corner=0.5, cx=0.4 * w, cy=0.45 * h)
    V[h - h // 10:, :] = 0.0
    return V


def expose(gray_float, forward_response, V):
    """Camera simulator: irradiance `gray_float` in [0, 1] through the vignette V, then the forward response, rounded to u8."""
    e = np.asarray(gray_float, np.float64) * np.asarray(V, np.float64)
    return np.clip(np.rint(forward_response(e)), 0, 255).astype(np.uint8)
