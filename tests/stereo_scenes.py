"""stereo_scenes.py -- hand-made keypoint scenes for Frame::ComputeStereoMatches (test infrastructure only), shared by
tests/test_stereo_ref_cpu.py (restatement against the C oracle, every keypoint's stage asserted) and tests/test_gpu_stereo_cases.py
(ivf_stereo_match against both).  Everything is drawn from fixed seeds.

Base pair: the left image is a dense smooth texture with values in [60, 190]; the right image is the left shifted by an integer
disparity d (right[x] = left[x + d]: a point at uL appears at uR = uL - d), cut from one wider texture so that no border is made up.
`noise` adds a seeded value in {-1, 0, 1} to every right pixel: the SAD of a true match is then > 0 and about the same everywhere, so
the median gate keeps the matches (with SAD 0 everywhere the median is 0 and Frame.cc:924 drops everything).  Keypoints are placed by
hand; a left keypoint and its right partner get a random 256-bit descriptor and a copy with k chosen bits flipped, everything else
independent draws (Hamming distance 128 +- 8 to anything: P(< 75) is below 1e-10 per pair).

A Scene is one image pair and its calls; a Call is one ivf_stereo_match with, for every left keypoint, the stage it was built to end
at (`stage`) and what else holds by construction (`checks`: lists of (left index, key, value), see test_stereo_ref_cpu.check_call).
"""
import numpy as np

F = np.float32
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])   # ivf_keypoint
BF, B = 40.0, 0.5                                   # maxD = bf / b = 80, exact in float32
MAXD = 80
PAD = 96
NLEVELS, SCALE_FACTOR = 8, 1.2
# (width, height, nfeatures): the row table H * (4 + 2 * 96) bytes fits 150 KB of LDS up to H = 783; neither height is a multiple of 4
SIZES = {"lds": (320, 203, 300), "global": (160, 801, 300)}
FAMILIES = ("hamming", "ties", "row_band", "octave_window", "disparity_range", "rounding", "alignment", "borders", "subpixel",
            "median_gate", "capacity", "n_right_max")


def scale_table():
    """mvScaleFactors / mvInvScaleFactors as ORBextractor.cc:428-447 builds them"""
    s = [F(1.0)]
    for _ in range(1, NLEVELS):
        s.append(F(s[-1] * F(SCALE_FACTOR)))
    s = np.array(s, F)
    return s, (F(1.0) / s).astype(F)


SCALE, INV_SCALE = scale_table()


def texture(h, w, seed):
    rng = np.random.default_rng(seed)
    a = rng.random((h + 4, w + 4))
    for _ in range(2):                                                    # 3 x 3 box twice: correlation length ~ 2 px
        hh, ww = a.shape[0] - 2, a.shape[1] - 2
        a = sum(a[i:i + hh, j:j + ww] for i in range(3) for j in range(3)) / 9.0
    z = (a - a.mean()) / a.std()
    return np.clip(np.rint(125.0 + 22.0 * z), 60, 190).astype(np.uint8)


def base_pair(w, h, d, seed, noise=True):
    tex = texture(h, w + 2 * PAD, seed)
    left = tex[:, PAD:PAD + w].copy()
    right = tex[:, PAD + d:PAD + d + w].copy()
    if noise:
        n = np.random.default_rng(seed + 1000).integers(-1, 2, size=right.shape)
        right = (right.astype(np.int16) + n).astype(np.uint8)
    return left, right


class Call:
    def __init__(self, name):
        self.name = name
        self.kl, self.dl, self.kr, self.dr = [], [], [], []
        self.stage = []
        self.checks = []

    def arrays(self):
        kl = np.zeros(len(self.kl), KP_DTYPE); kr = np.zeros(len(self.kr), KP_DTYPE)
        for a, src in ((kl, self.kl), (kr, self.kr)):
            for i, (x, y, o) in enumerate(src):
                a[i] = (x, y, 31.0 * float(SCALE[o]), 0.0, 1.0, o)
        dl = np.array(self.dl, np.uint8).reshape(-1, 32); dr = np.array(self.dr, np.uint8).reshape(-1, 32)
        return kl, dl, kr, dr


class Scene:
    def __init__(self, name, size, d, seed, noise=True):
        self.name = name
        self.w, self.h, self.nfeatures = SIZES[size]
        self.d = d
        self.img_left, self.img_right = base_pair(self.w, self.h, d, seed, noise)
        self.rng = np.random.default_rng(seed + 2000)
        self.calls = []

    def call(self, name):
        c = Call(name)
        self.calls.append(c)
        return c

    def desc(self, n=None):
        return self.rng.integers(0, 256, size=(32,) if n is None else (n, 32), dtype=np.uint8)

    def flipped(self, desc, k):
        """a copy of desc with k distinct randomly chosen bits flipped: Hamming distance exactly k"""
        bits = np.unpackbits(desc)
        bits[self.rng.choice(256, size=k, replace=False)] ^= 1
        return np.packbits(bits)

    def right(self, c, x, y, o, desc=None):
        c.kr.append((F(x), F(y), int(o)))
        c.dr.append(self.desc() if desc is None else desc)
        return len(c.kr) - 1

    def left(self, c, x, y, o, stage, desc=None):
        c.kl.append((F(x), F(y), int(o)))
        c.dl.append(self.desc() if desc is None else desc)
        c.stage.append(stage)
        return len(c.kl) - 1

    def pair(self, c, x, y, o, stage, k=20, dx=0.0, o_right=None, y_right=None, x_right=None):
        """left keypoint (x, y, octave o) and its partner at the true match (x - d) + dx, k descriptor bits apart"""
        iL = self.left(c, x, y, o, stage)
        xr = F(x) - F(self.d) + F(dx) if x_right is None else x_right
        iR = self.right(c, xr, y if y_right is None else y_right, o if o_right is None else o_right, self.flipped(c.dl[iL], k))
        if stage in ("matched", "gated"):
            c.checks.append((iL, "iR", iR))
        return iL, iR

    def fillers(self, c, n, y, o=0):
        """n right keypoints on row y with independent descriptors, anywhere a window fits"""
        xs = self.rng.integers(12, self.w - 12, size=n)
        for x in xs:
            self.right(c, float(x), y, o)


def level_xy(lx, ly, o):
    """extractor-like coordinates: integer level coordinates multiplied by the level's scale (ORBextractor.cc:1284-1288)"""
    return (F(lx), F(ly)) if o == 0 else (F(F(lx) * SCALE[o]), F(F(ly) * SCALE[o]))


def rows(scene, n, first=14, step=12):
    """n well separated rows: windows and octave-0 bands of keypoints on different rows do not touch"""
    assert first + step * (n - 1) < scene.h - 14, "scene too small for %d rows" % n
    return [first + step * i for i in range(n)]


# ---------------------------------------------------------------------------------------------------------------------------------
def hamming(size):
    """TH: bestDist < 75 goes on to the SAD; 75, 99 and 100 do not (100 never even replaces the initial TH_HIGH)"""
    s = Scene("hamming", size, 8, 11)
    c = s.call("thresholds")
    x = s.w // 2
    for y, k in zip(rows(s, 8), (0, 30, 73, 74, 75, 99, 100, 74)):
        s.pair(c, x + (y % 7), y, 0, "matched" if k < 75 else "hamming", k=k)
    return [s]


def ties(size):
    """two candidates at equal Hamming distance: the lower iR wins whatever its x -- next to each other, 64 and 66 entries apart in a
    listed row (64 < count <= 96: the same and another lane of the next 64-entry chunk) and 128 and 101 indices apart in a row that
    overflows the row cap (full scan by index).  The true match is at one candidate; the other sits 5 px off, so the true match is its last
    shift and the SAD ends at the edge of its range (edge_inc): the result tells who won."""
    s = Scene("ties", size, 8, 12)
    c = s.call("ties")
    x = s.w // 2
    ys = rows(s, 20, step=8)
    n = 0
    for n_fill, gap in ((0, 0), (70, 64), (70, 66), (130, 128), (130, 101)):
        for low_true, off in ((True, -5.0), (True, 5.0), (False, -5.0), (False, 5.0)):
            y = ys[n]; n += 1
            iL = s.left(c, x, y, 0, "matched" if low_true else "edge_inc")
            xt = F(x) - F(s.d)
            d_a = s.flipped(c.dl[iL], 33); d_b = s.flipped(c.dl[iL], 33)
            assert bytes(d_a) != bytes(d_b)
            before = min(3, n_fill)
            s.fillers(c, before, y)
            lo = s.right(c, xt if low_true else xt + F(off), y, 0, d_a)
            s.fillers(c, gap - 1 if gap else 0, y)
            hi = s.right(c, xt + F(off) if low_true else xt, y, 0, d_b)
            s.fillers(c, n_fill - before - max(gap - 1, 0), y)
            assert not gap or (lo // 64 != hi // 64 and hi - lo == gap)
            c.checks.append((iL, "iR", lo))
            c.checks.append((iL, "row_count", n_fill + 2))
    return [s]


def row_band(size):
    """vRowIndices: a right keypoint is a candidate on rows floor(y - r) .. ceil(y + r), r = 2 * scale[octave]; fractional y on both
    sides; bands clamped at row 0 and at row H - 1 (undefined in the reference, clamped by the library)"""
    out = []
    for o in (0, 3, 7):
        s = Scene("row_band_o%d" % o, size, 8, 13 + o)
        c = s.call("band")
        r = F(F(2.0) * SCALE[o])
        lx = int((s.w // 2) * float(INV_SCALE[o]))
        x = level_xy(lx, 0, o)[0]
        step = 2 * int(np.ceil(r)) + 16
        y0 = 30.3
        for i, which in enumerate(("minr", "maxr", "below", "above")):
            yr = F(y0 + i * step)
            maxr = int(np.ceil(F(yr + r))); minr = int(np.floor(F(yr - r)))
            row = {"minr": minr, "maxr": maxr, "below": minr - 1, "above": maxr + 1}[which]
            inside = which in ("minr", "maxr")
            iL, _ = s.pair(c, x, F(row + 0.7), o, "matched" if inside else "no_candidates", y_right=yr)
            c.checks.append((iL, "row_count", 1 if inside else 0))
        out.append(s)
    # clamped bands: an octave-7 right keypoint near the top / bottom edge.  A left keypoint of octave 6 on row 13 or 14 still has its
    # window inside level 6, so the clamped band's match is seen; at the bottom no left window fits inside the band: outside_domain
    s = Scene("row_band_clamped", size, 8, 21)
    c = s.call("clamped")
    x = level_xy(int((s.w // 2) * float(INV_SCALE[6])), 0, 6)[0]
    iL, _ = s.pair(c, x, F(13.6), 6, "matched", o_right=7, y_right=F(6.9))
    c.checks.append((iL, "row_count", 1))
    iL, _ = s.pair(c, x, F(s.h - 1 - 0.4), 6, "outside_domain", o_right=7, y_right=F(s.h - 1 - 6.9))
    c.checks.append((iL, "row_count", 1))
    iL, _ = s.pair(c, x, F(0.4), 1, "outside_domain", o_right=0, y_right=F(1.2))
    c.checks.append((iL, "row_count", 2))                                # the octave-7 band reaches row 0 as well
    out.append(s)
    return out


def octave_window(size):
    """kpR.octave in [levelL - 1, levelL + 1]; outside it the candidate is skipped and bestDist stays TH_HIGH"""
    s = Scene("octave_window", size, 8, 31)
    c = s.call("octaves")
    o = 2
    lx = int((s.w // 2) * float(INV_SCALE[o]))
    for i, do in enumerate((-2, -1, 0, 1, 2)):
        x, y = level_xy(lx + i, 20 + 18 * i, o)
        s.pair(c, x, y, o, "matched" if abs(do) <= 1 else "hamming", o_right=o + do)
    return [s]


def disparity_range(size):
    """uR in [uL - maxD, uL], both ends included, one float32 ulp outside each excluded"""
    out = []
    for d, name in ((79, "minU"), (1, "maxU")):
        s = Scene("disparity_%s" % name, size, d, 41 + d)
        c = s.call(name)
        ys = rows(s, 4)
        for i, x in enumerate((s.w - 30, s.w - 41)):
            uL = F(x)
            edge = F(uL - F(MAXD)) if name == "minU" else uL
            outside = np.nextafter(edge, F(-1e9) if name == "minU" else F(1e9), dtype=F)
            iL, _ = s.pair(c, uL, ys[2 * i], 0, "matched", x_right=edge)
            c.checks.append((iL, "bestinc", 1 if name == "minU" else -1))
            s.pair(c, uL, ys[2 * i + 1], 0, "hamming", x_right=outside)
        out.append(s)
    return out


def rounding(size):
    """round() is half away from zero: x = k + 0.5 gives k + 1 for even and odd k (round-half-even would give k for even k and move the
    best shift by one); upper octaves with extractor-like coordinates, level coordinates multiplied by the scale"""
    s = Scene("rounding", size, 8, 51)
    c = s.call("octave0_halves")
    x = s.w // 2
    for i, (y, k) in enumerate(zip(rows(s, 8), (x, x + 1, x + 2, x + 3, x, x + 1, x + 2, x + 3))):
        half_r = i >= 4                                                  # the partner on a .5 as well (even and odd k - d too)
        uL = F(k + 0.5)
        xr = F(k - s.d + 0.5) if half_r else F(k - s.d)
        iL, _ = s.pair(c, uL, F(y + 0.5), 0, "matched", x_right=xr)
        # scaleduL = k + 1, scaleduR0 = k - d (+ 1): the left window sits at k + 1, whose match is k + 1 - d
        c.checks.append((iL, "bestinc", 0 if half_r else 1))
    out = [s]
    for o in (1, 4, 7):
        s = Scene("rounding_o%d" % o, size, 8, 52 + o)
        c = s.call("extractor_like")
        lx = int((s.w // 2) * float(INV_SCALE[o]))
        ly0 = 16
        shift = int(round(8 * float(INV_SCALE[o])))
        for i in range(3):
            x, y = level_xy(lx + i, ly0 + 14 * i, o)
            xr = level_xy(lx + i - shift, 0, o)[0]
            s.pair(c, x, y, o, "matched", x_right=xr)
        out.append(s)
    return out


def alignment(size):
    """the SAD windows travel as whole dwords: all 16 combinations of (xl & 3, x0R & 3), at octave 0 and at octave 2"""
    out = []
    for o in (0, 2):
        s = Scene("alignment_o%d" % o, size, 8, 61 + o)
        c = s.call("xl_x0R")
        lx0 = int((s.w // 2) * float(INV_SCALE[o]))
        shift = int(round(8 * float(INV_SCALE[o])))
        seen = set()
        ly = 14
        for i in range(4):
            for j in (-1, 0, 1, 2):
                x, y = level_xy(lx0 + i, ly, o)
                xr = level_xy(lx0 + i - shift - j, 0, o)[0]
                iL, _ = s.pair(c, x, y, o, "matched", x_right=xr)
                if o == 0:
                    c.checks.append((iL, "bestinc", j))
                seen.add(((lx0 + i - 5) & 3, (lx0 + i - shift - j - 10) & 3))
                ly += 10 if o == 0 else 7
        assert len(seen) == 16
        out.append(s)
    return out


def borders(size):
    """endu = scaleduR0 + 11 < cols: == cols - 1 accepted, == cols rejected; scaleduR0 - 10 >= 0: == 10 accepted, 9 leaves the level"""
    out = []
    for o in (0, 2):
        s = Scene("borders_o%d" % o, size, 2, 71 + o)
        c = s.call("right_window")
        cols = int(np.floor(s.w * float(INV_SCALE[o]) + 0.5))
        shift = 2 if o == 0 else 1
        for i, (lxr, stage) in enumerate(((cols - 12, "matched"), (cols - 11, "right_border"), (10, "matched"), (9, "outside_domain"))):
            x, y = level_xy(lxr + shift, 16 + 14 * i, o)
            s.pair(c, x, y, o, stage, x_right=level_xy(lxr, 0, o)[0])
        c.checks.append((0, "cols", (o, cols)))
        out.append(s)
    return out


def symmetrise(img, cx, cy):
    """make rows cy-5..cy+5 mirror-symmetric about column cx over cx-11..cx+11"""
    for i in range(1, 12):
        img[cy - 5:cy + 6, cx + i] = img[cy - 5:cy + 6, cx - i]


def subpixel(size):
    """bestincR: +-4 accepted, +-5 rejected; negative disparity rejected; disparity exactly 0 clamped to 0.01"""
    s = Scene("subpixel", size, 8, 81)
    c = s.call("offsets")
    x = s.w // 2
    for y, dx in zip(rows(s, 6), (4, -4, 5, -5, 3, 0)):
        iL, _ = s.pair(c, x + (y % 5), y, 0, "matched" if abs(dx) < 5 else "edge_inc", dx=dx)
        c.checks.append((iL, "bestinc", -dx))
    out = [s]
    # the true match two pixels to the RIGHT of a candidate at uR == uL
    s = Scene("subpixel_negative", size, -2, 82)
    c = s.call("negative")
    ys = rows(s, 3)
    iL, _ = s.pair(c, x, ys[0], 0, "disparity", x_right=F(x))
    c.checks.append((iL, "bestinc", 2))
    iL, _ = s.pair(c, x + 9, ys[1], 0, "disparity", x_right=F(x + 8))
    c.checks.append((iL, "bestinc", 3))
    out.append(s)
    # identical images, patch mirror-symmetric about the keypoint's column: SAD(inc) == SAD(-inc), so dist1 == dist3, deltaR == 0 and the
    # disparity is exactly 0.  Four of the seven get + 4 on two mirror pixels of the right window (SAD 8, still symmetric): they keep
    # the median above 0, or the gate would drop everything.
    s = Scene("subpixel_zero", size, 0, 83, noise=False)
    c = s.call("clamp")
    ys = rows(s, 7)
    for i, y in enumerate(ys):
        symmetrise(s.img_left, x + 3 * i, y)
    s.img_right[:] = s.img_left
    for i, y in enumerate(ys):
        cx = x + 3 * i
        if i >= 3:
            s.img_right[y - 2, cx + 1] += 4
            s.img_right[y - 2, cx - 1] += 4
        iL, _ = s.pair(c, cx, y, 0, "matched", x_right=F(cx))
        c.checks += [(iL, "bestinc", 0), (iL, "sad", 8 if i >= 3 else 0), (iL, "clamp", None)]
    out.append(s)
    return out


def median_gate(size):
    """sort(vDistIdx); median = [size / 2]; keep dist < 1.5f * 1.4f * median.  Noise-free pair: the SAD at the true shift is 0, and
    adding delta to single non-centre pixels of the right window makes it exactly the sum of the deltas."""
    s = Scene("median_gate", size, 8, 91, noise=False)
    lists = (("odd", (3, 5, 7, 9, 40), (40,)),
             ("even", (4, 5, 10, 30), (30,)),                           # [size / 2] = 10: 21 keeps 10; the lower middle, 5, would drop it
             ("median_zero", (0, 0, 0, 5), (0, 0, 0, 5)),
             ("single", (9,), ()),
             ("f32_product", (10, 10, 21), (21,)),                      # 1.5f * 1.4f * 10 rounds to 21.0f exactly: 21 < 21 fails
             ("closed_form", (0, 6, 6, 6), ()),
             ("high_byte", (257, 270, 280, 290, 500, 620), (620,)))     # median 290 = 0x122: 257..280 and 500 share its high byte
    n_slots = sum(len(v) for _, v, _ in lists)
    per_row = max(1, (s.w - 60) // 36)
    slot = 0
    for name, values, dropped in lists:
        c = s.call(name)
        drop = list(dropped)
        for v in values:
            y = 14 + 12 * (slot // per_row); x = 40 + 36 * (slot % per_row); slot += 1
            assert y < s.h - 14 and x < s.w - 8
            xr = x - s.d
            rest = v
            for py in range(-5, 6):                                     # raster order, centre pixel excluded, 40 per pixel at most
                for px in range(-5, 6):
                    if rest and (px, py) != (0, 0):
                        dv = min(rest, 40); rest -= dv
                        s.img_right[y + py, xr + px] += dv
            gone = v in drop
            if gone:
                drop.remove(v)
            iL, _ = s.pair(c, x, y, 0, "gated" if gone else "matched")
            c.checks += [(iL, "sad", v), (iL, "bestinc", 0)]
            if v == 0 and not gone:
                c.checks.append((iL, "closed_form", None))
    assert slot == n_slots and s.img_right.max() <= 230
    return [s]


def capacity(size):
    """rows covered by exactly kRowCap = 96 right keypoints (listed), by 97 and by 300 (full scan), n_right > nfeatures; the partner is
    the highest index of its row"""
    s = Scene("capacity", size, 8, 101)
    c = s.call("row_cap")
    x = s.w // 2
    for y, n in zip(rows(s, 4, step=20), (96, 97, 300, 64)):
        s.fillers(c, n - 1, y)
        iL, iR = s.pair(c, x, y, 0, "matched")
        c.checks.append((iL, "row_count", n))
        assert iR == len(c.kr) - 1
    assert len(c.kr) > s.nfeatures
    # handle reuse: the same handles, a smaller right set and a smaller left set (the outputs are n_left long: what an earlier,
    # longer call left behind must not show)
    c2 = s.call("smaller")
    for y, n in zip(rows(s, 2, first=24, step=20), (5, 97)):
        s.fillers(c2, n - 1, y)
        iL, iR = s.pair(c2, x + 3, y, 0, "matched")
        c2.checks.append((iL, "row_count", n))
    return [s]


def n_right_max(size):
    """n_right = 65534, the largest the u16 row lists allow (0xffff is the matcher's `none`); the winners are 65533, 0 and 65532"""
    s = Scene("n_right_max", size, 8, 111)
    c = s.call("65534")
    n = 65534
    x = s.w // 2
    ys = rows(s, 3, first=20, step=30)
    left = [s.desc() for _ in ys]
    # fillers stay off the left keypoints' disparity range on their rows only by their descriptors: independent draws
    fx = s.rng.integers(12, s.w - 12, size=n); fy = s.rng.uniform(3.0, s.h - 4.0, size=n); fd = s.desc(n)
    c.kr = [(F(a), F(b), 0) for a, b in zip(fx, fy)]
    c.dr = list(fd)
    for y, dl, iR in zip(ys, left, (n - 1, 0, n - 2)):
        iL = s.left(c, x, y, 0, "matched", dl)
        c.kr[iR] = (F(x - s.d), F(y), 0)
        c.dr[iR] = s.flipped(dl, 20)
        c.checks.append((iL, "iR", iR))
    assert len(c.kr) == n
    return [s]


_BUILDERS = dict(hamming=hamming, ties=ties, row_band=row_band, octave_window=octave_window, disparity_range=disparity_range,
                 rounding=rounding, alignment=alignment, borders=borders, subpixel=subpixel, median_gate=median_gate, capacity=capacity,
                 n_right_max=n_right_max)
_CACHE = {}


def build(family, size):
    """the scenes of one family at one size (built once per process)"""
    key = (family, size)
    if key not in _CACHE:
        _CACHE[key] = _BUILDERS[family](size)
    return _CACHE[key]


def evaluate(scene):
    """the oracle extractor's pyramids of the scene's images and, for every call, its arrays, the restatement's answer and the C
    oracle's (computed once per scene and left unchanged)"""
    if getattr(scene, "_eval", None) is None:
        import oracle_lib as O
        import stereo_ref as SR
        eL = O.Extractor(scene.nfeatures, SCALE_FACTOR, NLEVELS, 20, 7); eR = O.Extractor(scene.nfeatures, SCALE_FACTOR, NLEVELS, 20, 7)
        eL(scene.img_left); eR(scene.img_right)
        t = eL.tables()
        pl = [eL.pyramid(l) for l in range(NLEVELS)]; pr = [eR.pyramid(l) for l in range(NLEVELS)]
        assert np.array_equal(t["scale"], SCALE) and np.array_equal(t["inv_scale"], INV_SCALE)
        calls = []
        for c in scene.calls:
            kl, dl, kr, dr = c.arrays()
            ref = SR.stereo_match(pl, pr, t["scale"], t["inv_scale"], kl, dl, kr, dr, BF, B)
            our, odp = O.stereo_match(eL, eR, kl, dl, kr, dr, BF, B)
            calls.append(dict(call=c, arrays=(kl, dl, kr, dr), ref=ref, oracle=(our, odp)))
        scene._eval = dict(pyr_left=pl, pyr_right=pr, tables=t, calls=calls)
    return scene._eval
