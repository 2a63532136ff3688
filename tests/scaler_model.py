"""Real-valued model of the scaling front-end, the error bound that relates the fixed-point specification to
it, and the hard content the scaler's tests run on.  Shared by tests/test_frontend_oracle.py (the CPU statement) and
tests/test_gpu_scaler_edges.py (the kernel).

The model starts from the 8-bit planes the specification's integer colour matrix produces (that matrix is checked against real
BT.601 in test_frontend_oracle.py) and does everything after it in float64: output centres at the specification's 16.16
positions, bicubic weights (B = 0, C = 0.6, widened by the scale, edge replication) normalised in double, the horizontal pass
clamped to the 15-bit intermediate's range, limited-range expansion in real arithmetic, and the vertical pass clamped to
0..255 and NOT rounded.  It shares nothing with the integer code but the positions and the filter family, so a misreading of
the specification that the kernel and oracle/frontend_oracle.c make together (a clamp in the wrong place, a rounding constant)
shows up against it."""
import numpy as np

ONE = 65536
T_MAX = 32767 / 128            # the 15-bit intermediate's largest value, in sample units
G_LUMA, G_CHROMA = 255 / 219, 255 / 224
LIMITED_LEVELS = (0, 15, 16, 235, 236, 240, 255)
# the content of sources above 4 Mpx (the model's cost grows with the source)
LARGE_SOURCE_KINDS = ["noise", "checker1", "impulses_on_black", "primaries", "levels"]

# (format (0 RGB24, 1 YUV420P), source w, h, full range, target w, h)
# every tile shape fits each of these in an MI355X's 160 KiB of LDS per CU
TILE_GEOMETRIES = [
    (0, 640, 480, True, 320, 240),
    (1, 720, 576, False, 640, 480),
    (1, 1280, 720, True, 320, 176),
    (0, 97, 61, True, 48, 32),          # odd width: the RGB byte path; partial tiles
    (0, 3, 5, True, 1024, 1024),
    (1, 2, 2, True, 1024, 1024),        # a one-sample chroma plane
    (1, 350, 286, True, 320, 240),      # pitches 350 and 175: the YUV byte path; the V plane at an odd offset
]
# large sources: the create code's own choice of the smaller tiles, banks up to 64 taps
EXTREME_GEOMETRIES = [
    (0, 1920, 1080, True, 320, 240),    # a 48-tap chroma bank (RGB chroma: 1920 -> 160)
    (0, 2560, 1440, True, 320, 240),    # 64 taps: exactly 16x
    (1, 3000, 2000, False, 320, 240),
    (1, 6000, 4000, True, 384, 256),    # 63 taps both ways
    (1, 16384, 64, True, 1024, 16),
    (1, 64, 16384, True, 16, 1024),
]


def xinc(src, dst):
    return ((src << 16) + dst // 2) // dst


def cubic(x, B=0.0, C=0.6):
    x = np.abs(x)
    w1 = ((12 - 9 * B - 6 * C) * x ** 3 + (-18 + 12 * B + 6 * C) * x ** 2 + (6 - 2 * B)) / 6
    w2 = ((-B - 6 * C) * x ** 3 + (6 * B + 30 * C) * x ** 2 + (-12 * B - 48 * C) * x + (8 * B + 24 * C)) / 6
    return np.where(x < 1, w1, np.where(x < 2, w2, 0.0))


def model_bank(src, dst):
    """(positions (dst, n) int64, weights (dst, n) float64): every source position within the widened support of each output
    centre, unclamped; each row of weights sums to 1"""
    xi = xinc(src, dst)
    scale = max(xi, ONE) / ONE
    c = (np.arange(dst, dtype=np.int64) * xi + ((xi - ONE) >> 1)) / ONE
    lo = np.floor(c - 2 * scale).astype(np.int64)
    n = int(np.ceil(4 * scale)) + 2
    pos = lo[:, None] + np.arange(n)[None, :]
    w = cubic((pos - c[:, None]) / scale)
    return pos, w / w.sum(axis=1, keepdims=True)


def _pass(plane, dst, axis):
    """one separable pass along `axis` (1: horizontal, 0: vertical) with edge replication"""
    src = plane.shape[axis]
    pos, w = model_bank(src, dst)
    idx = np.clip(pos, 0, src - 1)
    shape = (plane.shape[0], dst) if axis == 1 else (dst, plane.shape[1])
    acc = np.zeros(shape)
    for k in range(pos.shape[1]):
        if axis == 1:
            acc += plane[:, idx[:, k]] * w[:, k]
        else:
            acc += plane[idx[:, k], :] * w[:, k, None]
    return acc


def model_plane(plane, dw, dh, mode=0):
    """plane: 8-bit samples (h, w) -> (dh, dw) float64, unrounded.  mode: 0 full range, 1 limited-range luma, 2 limited chroma"""
    t = np.clip(_pass(plane, dw, 1), 0.0, T_MAX)
    if mode == 1:
        t = np.minimum((t - 16) * G_LUMA, T_MAX)
    elif mode == 2:
        t = np.minimum((t - 128) * G_CHROMA + 128, T_MAX)
    return np.clip(_pass(t, dh, 0), 0.0, 255.0)


def rgb_planes(pic, w, h):
    """the specification's integer BT.601 full-range matrix: RGB24 -> 8-bit Y, Cb, Cr at full resolution"""
    p = pic.reshape(h, w, 3).astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = np.clip(((-11059 * r - 21709 * g + 32768 * b + 32768) >> 16) + 128, 0, 255)
    cr = np.clip(((32768 * r - 27439 * g - 5329 * b + 32768) >> 16) + 128, 0, 255)
    return y.astype(np.uint8), cb.astype(np.uint8), cr.astype(np.uint8)


def yuv_planes(pic, w, h):
    n, c = w * h, (w // 2) * (h // 2)
    return pic[:n].reshape(h, w), pic[n:n + c].reshape(h // 2, w // 2), pic[n + c:n + 2 * c].reshape(h // 2, w // 2)


def model_convert(fmt, sw, sh, full, dw, dh, pic):
    """one picture -> the model's (Y (dh, dw), Cr, Cb (dh/2, dw/2)), float64"""
    if fmt == 0:
        y, cb, cr = rgb_planes(pic, sw, sh)
        lm = cm = 0
    else:
        y, cb, cr = yuv_planes(pic, sw, sh)
        lm, cm = (0, 0) if full else (1, 2)
    return (model_plane(y, dw, dh, lm), model_plane(cr, dw // 2, dh // 2, cm), model_plane(cb, dw // 2, dh // 2, cm))


def nv21_planes(frame, dw, dh):
    """an NV21 frame -> (Y, Cr, Cb) as float64 planes"""
    f = np.asarray(frame).astype(np.float64)
    n = dw * dh
    return f[:n].reshape(dh, dw), f[n::2].reshape(dh // 2, dw // 2), f[n + 1::2].reshape(dh // 2, dw // 2)


# ---------------------------------------------------------------- the error bound
def bank_error(src, dst, taps, left, coef):
    """largest per-output sum over source positions of |coef / 16384 - w| (integer bank against the model's weights)"""
    pos, w = model_bank(src, dst)
    base = np.minimum(left.astype(np.int64), pos[:, 0])
    width = int(max((left + taps - base).max(), (pos[:, -1] + 1 - base).max()))
    d = np.zeros((dst, width))
    rows = np.arange(dst)[:, None]
    d[rows, left[:, None] - base[:, None] + np.arange(taps)[None, :]] += coef / 16384.0
    d[rows, pos - base[:, None]] -= w
    return float(np.abs(d).sum(axis=1).max())


def expansion_error(mode):
    """largest |integer range expansion - real one| over every 15-bit intermediate, in sample units (0 without expansion)"""
    if mode == 0:
        return 0.0
    t = np.arange(32768, dtype=np.int64)
    if mode == 1:
        got = (np.minimum(t, 30189) * 19077 - 39057361) >> 14
        want = np.minimum((t / 128 - 16) * G_LUMA, T_MAX)
    else:
        got = (np.minimum(t, 30775) * 4663 - 9289992) >> 12
        want = np.minimum((t / 128 - 128) * G_CHROMA + 128, T_MAX)
    return float(np.abs(got / 128 - want).max())


def plane_bound(src_w, src_h, dw, dh, mode, filter_fn):
    """max |fixed point - model| for one plane, derived from the banks (filter_fn(src, dst) -> (taps, left, coef)):

        0.5 + T_MAX E_v + A_v (g (255 E_h + 1/128) + max(1/128, D))

    0.5 is the final rounding; E_v, E_h the vertical / horizontal banks' coefficient error (bank_error); A_v the largest sum
    of |w| of the vertical bank (what an error in the intermediates is amplified by); 255 E_h + 1/128 the horizontal pass's
    error (coefficients, then the floor of >> 7); g the range expansion's slope (1 without one); D the expansion's own error
    against the real map (the floor of its shift, and constants rounded to 14 / 12 bits: 1.63/128 at most, for chroma at 0).
    The clamps are 1-Lipschitz and do not add to it."""
    e_h = bank_error(src_w, dw, *filter_fn(src_w, dw))
    e_v = bank_error(src_h, dh, *filter_fn(src_h, dh))
    a_v = float(np.abs(model_bank(src_h, dh)[1]).sum(axis=1).max())
    g = (1.0, G_LUMA, G_CHROMA)[mode]
    return 0.5 + T_MAX * e_v + a_v * (g * (255 * e_h + 1 / 128) + max(1 / 128, expansion_error(mode)))


def convert_bounds(fmt, sw, sh, full, dw, dh, filter_fn):
    """(bound for Y, bound for Cr and Cb) of one geometry"""
    csw, csh = (sw, sh) if fmt == 0 else (sw // 2, sh // 2)
    lm, cm = (0, 0) if (fmt == 0 or full) else (1, 2)
    return plane_bound(sw, sh, dw, dh, lm, filter_fn), plane_bound(csw, csh, dw // 2, dh // 2, cm, filter_fn)


# ---------------------------------------------------------------- hard content
def _marks(src, dst, step):
    """source positions next to the output positions where bands / tiles start (every `step` outputs), and both ends"""
    m = np.arange(0, dst + 1, step)
    s = np.floor((m - 0.5) * src / dst).astype(np.int64)
    return np.unique(np.clip(np.concatenate([s, s + 1, [0, src - 1]]), 0, src - 1))


def _impulses(h, w, rows, cols, bright):
    p = np.full((h, w), 0 if bright else 255, np.uint8)
    p[np.ix_(rows, cols)] = 255 if bright else 0
    return p


def kinds_for(sw, sh):
    return LARGE_SOURCE_KINDS if sw * sh > 4_000_000 else None


def hard_pictures(fmt, sw, sh, dw, dh, limited=False, seed=0, kinds=None):
    """[(name, picture bytes)] of content that drives the clamps: noise, 0/255 checkerboards of period 1, 2, 3 and 8, isolated
    bright / dark samples at the picture's first and last rows and columns and at band and tile boundaries (all four tile
    shapes' boundaries: multiples of 16 columns and 8 rows of the output), hard edges, primaries and secondaries (Cb and Cr at
    1 and 255), and for limited-range YUV planes built from the levels around the range's ends"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:sh, 0:sw]
    cyy, cxx = np.mgrid[0:sh // 2, 0:sw // 2]

    def checker(x, y, p):
        return ((((x // p) + (y // p)) % 2) * 255).astype(np.uint8)

    def cells(h, w, size, values):
        v = np.asarray(values, np.uint8)
        grid = rng.integers(0, len(v), ((h + size - 1) // size, (w + size - 1) // size))
        return v[np.repeat(np.repeat(grid, size, 0), size, 1)[:h, :w]]

    names = ["noise", "checker1", "checker2", "checker3", "checker8", "impulses_on_black", "impulses_on_white", "edges", "primaries"]
    if fmt == 1 and limited:
        names.append("levels")
    out = []
    for name in names:
        if kinds is not None and name not in kinds:
            continue
        if fmt == 0:
            if name == "noise":
                pic = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
            elif name.startswith("checker"):
                p = int(name[7:])
                c = checker(xx, yy, p)
                # periods 1 and 8: full-contrast grey; 2 and 3: yellow against blue (Cb 1 against 255)
                pic = np.stack([c, c, c if p in (1, 8) else 255 - c], axis=-1)
            elif name.startswith("impulses"):
                rows = np.union1d(_marks(sh, dh, 8), _marks(sh, dh // 2, 4))
                cols = np.union1d(_marks(sw, dw, 16), _marks(sw, dw // 2, 8))
                pic = np.repeat(_impulses(sh, sw, rows, cols, name.endswith("black"))[..., None], 3, axis=-1)
            elif name == "edges":
                e = ((((xx * 7) // sw + (yy * 5) // sh) % 2) * 255).astype(np.uint8)
                pic = np.stack([e, 255 - e, e], axis=-1)
            else:   # the corners of the RGB cube in cells of 1 to 4 pixels
                corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
                size = 1 + int(rng.integers(0, 4))
                idx = cells(sh, sw, size, np.arange(8))
                pic = corners[idx]
            out.append((name, np.ascontiguousarray(pic).reshape(-1)))
            continue
        ch, cw = sh // 2, sw // 2
        if name == "noise":
            y, u, v = rng.integers(0, 256, (sh, sw), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8)
        elif name.startswith("checker"):
            p = int(name[7:])
            y, u = checker(xx, yy, p), checker(cxx, cyy, p)
            v = 255 - u
        elif name.startswith("impulses"):
            bright = name.endswith("black")
            rows, cols = _marks(sh, dh, 8), _marks(sw, dw, 16)
            crows, ccols = _marks(ch, dh // 2, 4), _marks(cw, dw // 2, 8)
            y = _impulses(sh, sw, rows, cols, bright)
            u, v = _impulses(ch, cw, crows, ccols, bright), _impulses(ch, cw, crows, ccols, not bright)
        elif name == "edges":
            y = ((((xx * 7) // sw + (yy * 5) // sh) % 2) * 255).astype(np.uint8)
            u = ((((cxx * 5) // cw + (cyy * 3) // ch) % 2) * 255).astype(np.uint8)
            v = 255 - u
        elif name == "primaries":
            size = 1 + int(rng.integers(0, 4))
            y, u, v = cells(sh, sw, 2 * size, (0, 255)), cells(ch, cw, size, (0, 255)), cells(ch, cw, size, (0, 255))
        else:   # levels: single samples in the top half, blocks of five in the bottom half
            def lv(h, w):
                return np.concatenate([cells(h // 2, w, 1, LIMITED_LEVELS), cells(h - h // 2, w, 5, LIMITED_LEVELS)])
            y, u, v = lv(sh, sw), lv(ch, cw), lv(ch, cw)
        out.append((name, np.concatenate([y.ravel(), u.ravel(), v.ravel()]).astype(np.uint8)))
    return out
