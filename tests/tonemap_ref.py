"""The display stage in numpy: csrc/host/tonemap.h restated, float32 / float64 in the order the header writes, written
apart from it -- the trimming as an intersection of intervals of the cumulative counts, not as the header's two walks -- plus a float64
model of the curves and the transfer function: the same expressions, with the header's float32 constants, evaluated in double from the
float32 operands c and exposure.  The model is what the float32 statement rounds; their distance is that rounding alone."""
import numpy as np

F = np.float32
D = np.float64
FLT_MAX = np.finfo(np.float32).max
N_BINS = 256
CLAMP, REINHARD, ACES, HABLE = 0, 1, 2, 3
LINEAR, SRGB = 0, 1
ADAPTED, METERED = 1, 2
CURVES = {"clamp": CLAMP, "reinhard": REINHARD, "aces": ACES, "hable": HABLE}
TRANSFERS = {"linear": LINEAR, "srgb": SRGB}
HABLE_CONSTANTS = tuple(F(v) for v in (0.15, 0.50, 0.10, 0.20, 0.02, 0.30))
SRGB_EXPONENT = F(1.0) / F(2.4)
CURVE_MAX_INPUT = 2.0 ** 32                                                    # the rational curves take min(x, 2^32): x^2 stays finite
DEFAULTS = dict(curve="aces", transfer="srgb", auto=True, exposure_scale=1.0, ev_bias=0, white=4.0, key=0.18, low_fraction=0.5, high_fraction=0.02, alpha=1.0)


def luminance(image):
    c = np.asarray(image, F)
    with np.errstate(all="ignore"):
        return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def luminance_bin(y):
    """the bin of each float32 luminance, -1 where it is not counted"""
    y = np.ascontiguousarray(y, F)
    with np.errstate(invalid="ignore"):
        counted = (y > 0) & (y <= FLT_MAX)
    b = (y.view(np.uint32) >> np.uint32(20)).astype(np.int64) - ((127 - 16) << 3)
    return np.where(counted, np.clip(b, 0, N_BINS - 1), -1)


def histogram(image):
    b = luminance_bin(luminance(image)).ravel()
    return np.bincount(b[b >= 0], minlength=N_BINS).astype(np.uint32), int((b < 0).sum())


def trimmed(counts, low_fraction, high_fraction):
    """what the trimming leaves of every bin: the counted pixels in luminance order are [0, N); [floor(low N), N - floor(high N)) stay"""
    c = [int(v) for v in counts]
    n = sum(c)
    first = int(np.floor(D(F(low_fraction)) * D(n)))
    last = n - int(np.floor(D(F(high_fraction)) * D(n)))
    left, start = [], 0
    for v in c:
        left.append(max(0, min(start + v, last) - max(start, first)))
        start += v
    return left, n


def meter(counts, low_fraction, high_fraction):
    """(m or None, N)"""
    left, n = trimmed(counts, low_fraction, high_fraction)
    den = sum(left)
    if den == 0:
        return None, n
    num2 = sum(v * (2 * i + 1) for i, v in enumerate(left))
    return (D(num2) * D(0.5)) / D(den), n


def adapt(m_adapted, have, m, alpha):
    return D(m_adapted) + (D(m) - D(m_adapted)) * D(F(alpha)) if have else D(m)


def index_luminance(m):
    q = D(m) / D(8.0) - D(16.0)
    f = np.floor(q)
    return np.ldexp(D(1.0) + (q - f), int(f))


def exposure_of(metered, exposure_scale, ev_bias):
    return (F(metered) * F(np.ldexp(D(1.0), int(ev_bias)))) * F(exposure_scale)


def auto_exposure(m_adapted, key, exposure_scale, ev_bias):
    return exposure_of(F(D(F(key)) / index_luminance(m_adapted)), exposure_scale, ev_bias)


def _hable_partial(x, T):
    A, B, C, Dd, E, Fc = (T(v) for v in HABLE_CONSTANTS)
    return ((x * (A * x + C * B) + Dd * E) / (x * (A * x + B) + Dd * Fc)) - E / Fc


def _curve(x, curve, white, T):
    """the header's expressions in the type T on x >= 0"""
    w = T(F(white))
    if curve == REINHARD:
        return (x * (T(1.0) + x / (w * w))) / (T(1.0) + x)
    if curve == ACES:
        return (x * (T(F(2.51)) * x + T(F(0.03)))) / (x * (T(F(2.43)) * x + T(F(0.59))) + T(F(0.14)))
    if curve == HABLE:
        return _hable_partial(x, T) / _hable_partial(w, T)
    return x


def _transfer(y, transfer, T):
    if transfer == LINEAR:
        return y
    y = np.where(y < T(1.0), y, T(1.0))
    return np.where(y <= T(F(0.0031308)), T(F(12.92)) * y, T(F(1.055)) * np.power(y, T(SRGB_EXPONENT)) - T(F(0.055)))


def map_channels(rgb, exposure, curve, transfer, white, T=F):
    """rgb float32 (..., 3) -> the curve and the transfer in the type T (F: the statement; D: the model)"""
    with np.errstate(all="ignore"):
        x = np.asarray(rgb, F).astype(T) * T(F(exposure))
        x = np.where(x > 0, x, T(0.0))
        if curve != CLAMP:
            x = np.where(x < T(CURVE_MAX_INPUT), x, T(CURVE_MAX_INPUT))
        y = np.asarray(_curve(x, curve, white, T), T)
        y = np.where(y == y, y, T(0.0))
        return np.asarray(_transfer(y, transfer, T), T)


def pack(rgb):
    """Vec4ToUint of float32 (..., 3)"""
    c = np.asarray(rgb, F)
    with np.errstate(invalid="ignore"):
        f = F(255.0) * np.where(c < F(1.0), c, F(1.0))
        f = np.where(f < F(0.0), F(0.0), f)
    b = f.astype(np.int32).astype(np.uint32) & np.uint32(0xFF)
    return (np.uint32(255) << np.uint32(24)) + (b[..., 2] << np.uint32(16)) + (b[..., 1] << np.uint32(8)) + b[..., 0]


def pack_reference(image):
    """Vec4ToUint of an image as cgpt_read_pixels packs it"""
    return pack(np.asarray(image, F)[..., :3])


class State:
    """what a context keeps between auto-exposure calls"""
    def __init__(self, adapted=0.0, valid=False):
        self.adapted, self.valid = D(adapted), bool(valid)


def tonemap(image, state=None, **kw):
    """The whole stage on a (rows, width, 4) float32 image.  Returns (rgba float32, pixels uint32, info dict or None); `state` (State) is
    updated as the context's is.  Keywords as DEFAULTS; curve / transfer by name or number."""
    p = dict(DEFAULTS, **kw)
    curve = CURVES[p["curve"]] if isinstance(p["curve"], str) else p["curve"]
    transfer = TRANSFERS[p["transfer"]] if isinstance(p["transfer"], str) else p["transfer"]
    image = np.asarray(image, F)
    info = None
    exposure = exposure_of(1.0, p["exposure_scale"], p["ev_bias"])
    if p["auto"]:
        state = state if state is not None else State()
        counts, n_ignored = histogram(image)
        m, n = meter(counts, p["low_fraction"], p["high_fraction"])
        valid = ADAPTED if state.valid else 0
        if m is not None:
            state.adapted, state.valid = adapt(state.adapted, state.valid, m, p["alpha"]), True
            valid = ADAPTED | METERED
        if state.valid:
            exposure = auto_exposure(state.adapted, p["key"], p["exposure_scale"], p["ev_bias"])
        info = dict(mean_index=D(0.0) if m is None else m, adapted_index=state.adapted if state.valid else D(0.0), exposure=exposure, valid=valid, n_counted=n,
                    n_ignored=n_ignored, histogram=counts)
    rgb = map_channels(image[..., :3], exposure, curve, transfer, p["white"], F)
    rgba = np.concatenate([rgb, np.ones(rgb.shape[:-1] + (1,), F)], axis=-1)
    return rgba, pack(rgb), info


def model(image, exposure, **kw):
    """the float64 model's (..., 3) channels for the float32 exposure the stage used"""
    p = dict(DEFAULTS, **kw)
    curve = CURVES[p["curve"]] if isinstance(p["curve"], str) else p["curve"]
    transfer = TRANSFERS[p["transfer"]] if isinstance(p["transfer"], str) else p["transfer"]
    return map_channels(np.asarray(image, F)[..., :3], exposure, curve, transfer, p["white"], D)


CODE = 2.0 ** -8                                                               # about one step of the packed pixel (1 / 255)


def relative_deviation(got, want):
    """max of |got - want| / max(|want|, CODE): the relative deviation of the encoded channels, with values below one output code
    measured against that code.  A purely relative measure has no bound there: Hable's curve is a difference that cancels towards 0
    (absolute error ~ 2^-24 over h(white) whatever y is) and denormal inputs carry a few bits, so the float32 statement itself is
    arbitrarily far from its model in relative terms, while the display cannot tell the two apart."""
    got, want = np.asarray(got, D), np.asarray(want, D)
    assert np.isfinite(want).all() and np.isfinite(got).all()
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), CODE)))
