"""Inputs of the warp tests whose source coordinates lie on, or a hair beside, integers - the only place where a small
arithmetic slip in ``int(tx), int(ty)`` and the strict test ``0 < t < size`` changes a canvas byte (DESIGN.md "K3").
Built once per session and shared: read-only.  tests/test_warp_integer_inputs.py asserts, on the CPU and from
oracle/warp_fast_spec.py alone, that every input reaches its edge; tests/test_gpu_warp_integer.py holds the kernels to the
oracle on them, byte for byte.

Every float32 cell is given by its FORWARD matrix (source -> canvas, what ``local_warp`` takes), chosen so that the float32
inverse the reference stores back is known exactly: ``exact_inverse_f32`` inverts the float32 entries in rational arithmetic
and rounds once, and the builder asserts that ``numpy.linalg.inv`` gives those bits.

A sweep cell maps the canvas to the source by ``t = w (L (x, y) + K) + (A, B)`` with ``w = m (1 + s 2^-e)``, ``L`` the identity,
a quarter turn or a shear with integer entries, ``K`` integers and ``A = -s m u_c 2^-e``: the coordinate is ``m u`` plus the
fraction ``s m 2^-e (u - u_c)``, which walks by ``m 2^-e`` per pixel through zero at ``u = u_c``.  Its forward matrix is
``[[L^-1, -L^-1 ((A, B) + w K)], [p, q, w]]``: the scale sits in the third component, so every coordinate is a real division.
``u_c`` is placed so that the band of fractions between half a doubt window and two windows lies on the cell's far corner.

The launcher gives a canvas to the float32-estimate kernel only when the mesh's MEAN cell is at most 128 px on both axes
(``takes_estimate_kernel``).  The cells here are 254 px, the largest span a record takes, so every mesh carries further cells
of 1 px beyond the canvas edge (``_pad_axis``) that bring its mean down; the case ``coarse`` leaves them out and so runs the
all-float64 strips under every context."""
from fractions import Fraction

import numpy as np

from oracle import apap_oracle as O
from oracle import warp_fast_spec as S

CELL = S.MAX_SPAN                   # 254: the largest span a record takes
# where the unflagged band next to the doubt window lies, in pixels from the crossing and per unit of 2^e: the window of a
# 254 px cell is about 1.5e-4 m px (fast_record: E32 = 9.5 x 2^-24 x 128 m), the band reaches from 0.5 to 2 windows
BAND_MID = 1.9e-4
FAR = 120                           # |dx|, |dy| from the anchor that count as the cell's far corner

_cases = {}
_classes = {}


def picture(h, w):
    """Any two of a pixel's eight neighbours differ from it in every channel and no pixel is black: a truncation to the
    wrong neighbour, or a bounds test that lets a pixel in or out, changes the bytes."""
    x, y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    img = np.empty((h, w, 3), np.uint8)
    img[..., 0] = (x + 2 * y) & 255
    img[..., 1] = (2 * x + y + 64 * ((x >> 8) + 2 * (y >> 8))) & 255
    img[..., 2] = (3 * x + 5 * y) % 251 + 1
    return img


def _round_f32(fr):
    """The float32 nearest to a Fraction (ties cannot be told apart from near-ties here and do not occur)."""
    v = np.float32(float(fr))
    best = min((v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))),
               key=lambda c: abs(Fraction(float(c)) - fr))
    return best


def exact_inverse_f32(H):
    """(3, 3) float32 forward matrix -> its inverse, computed exactly and rounded to float32 once."""
    a = [[Fraction(float(v)) for v in row] for row in np.asarray(H, np.float32)]
    cof = lambda r, c: a[(r + 1) % 3][(c + 1) % 3] * a[(r + 2) % 3][(c + 2) % 3] - a[(r + 1) % 3][(c + 2) % 3] * a[(r + 2) % 3][(c + 1) % 3]  # noqa: E731
    det = sum(a[0][c] * cof(0, c) for c in range(3))
    assert det != 0
    return np.array([[_round_f32(cof(c, r) / det) for c in range(3)] for r in range(3)], np.float32)


def checked_inverse(H):
    """The designed float32 inverses of a grid of forward matrices, asserted to be what numpy's inverse gives - bit for bit,
    once the zeros have taken numpy's signs (a zero of the rational inverse has none; LAPACK leaves -0 in a turned cell)."""
    H = np.asarray(H, np.float32)
    hinv = np.empty_like(H)
    for r in range(H.shape[0]):
        for c in range(H.shape[1]):
            hinv[r, c] = exact_inverse_f32(H[r, c])
    lapack = O.invert_cells_f32(H)
    assert np.array_equal(hinv, lapack), "LAPACK's float32 inverse is not the designed one"
    hinv = np.where(hinv == 0, lapack, hinv)
    assert hinv.tobytes() == lapack.tobytes()
    assert hinv.tobytes() == np.linalg.inv(H.astype(np.float64)).astype(np.float32).tobytes(), "numpy's float64 inverse is not the designed one"
    return hinv


IDENT = ((1, 0), (0, 1))
TURN = ((0, -1), (1, 0))            # u = -y, v = x: the sweep of tx runs along dy
SHEAR = ((1, 1), (0, 1))            # u = x + y: twice the reach of the estimate on the same cell


def sweep_cell(m, e, s, corner, L=IDENT, K=(0, 0), persp=(0.0, 0.0), mid=None):
    """Forward matrix of one sweep cell (see the module's text).  ``corner``: the canvas point (x, y), relative to the
    offsets, on which the unflagged band is centred."""
    w = m * (1.0 + s * 2.0 ** -e)
    mid = round(BAND_MID * 2.0 ** e) if mid is None else mid
    (l00, l01), (l10, l11) = L
    u = l00 * corner[0] + l01 * corner[1] + K[0]
    v = l10 * corner[0] + l11 * corner[1] + K[1]
    A = -s * m * (u - mid) * 2.0 ** -e
    B = -s * m * (v - mid) * 2.0 ** -e
    det = l00 * l11 - l01 * l10
    assert det in (1, -1)
    i00, i01, i10, i11 = l11 / det, -l01 / det, -l10 / det, l00 / det
    a, b = A + w * K[0], B + w * K[1]
    H = np.array([[i00, i01, -(i00 * a + i01 * b)], [i10, i11, -(i10 * a + i11 * b)], [persp[0], persp[1], w]])
    H32 = H.astype(np.float32)
    assert np.float32(w) == w and (K != (0, 0) or np.array_equal(H32.astype(np.float64), H)), "the cell is not a float32 matrix"
    return H32


def integer_cell(c, A, B):
    """A forward matrix whose float32 inverse is exactly ``c [[1, 0, A], [0, 1, B], [0, 0, 1]]``: the coordinates are the
    integers x + A, y + B, each the quotient of a division by c.  1 / c is no float32 for c = 3, 5, 7, so the entries are
    searched among the neighbours of the rounded ones; None when there are none."""
    want = np.array([[c, 0, c * A], [0, c, c * B], [0, 0, c]], np.float32)
    if c == 1:
        return np.array([[1, 0, -A], [0, 1, -B], [0, 0, 1]], np.float32)
    step = lambda v, k: v if k == 0 else step(np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf)), k - np.sign(k))  # noqa: E731
    p0 = np.float32(1.0 / c)
    for kp in (0, 1, -1):
        for kr in (0, 1, -1):
            p, r = step(p0, kp), step(p0, kr)
            if _round_f32(1 / Fraction(float(p))) != c or _round_f32(1 / Fraction(float(r))) != c:
                continue
            H = np.array([[p, 0, 0], [0, p, 0], [0, 0, r]], np.float32)
            found = True
            for row, t in ((0, A), (1, B)):
                a0 = np.float32(-c * t * float(p) * float(r))
                for ka in (0, 1, -1, 2, -2):
                    a = step(a0, ka)
                    if _round_f32(-Fraction(float(a)) / (Fraction(float(p)) * Fraction(float(r)))) == np.float32(c * t):
                        H[row, 2] = a
                        break
                else:
                    found = False
            if found and np.array_equal(exact_inverse_f32(H), want):
                return H
    return None


def _center(rng, h, w):
    c = rng.integers(1, 256, (h, w, 3), dtype=np.uint8)
    c[rng.integers(0, 4, (h, w)) == 0] = 0          # black centre pixels: the blend's other branch
    return c


FAST_MEAN_CELL = 128        # warp_impl (apap_kernels.hip): the estimate kernel runs when final_w / mesh_cols and final_h / mesh_rows
                            # (integer divisions by the numbers of cells) are at most this, else the all-float64 strips


def takes_estimate_kernel(case):
    """The launcher's choice between ``k_warp_fast`` and ``k_warp_rows`` for a context with ``warp_fast=1`` and strips, restated:
    a mesh whose MEAN cell is at most 128 px on both axes, edge tables of at most 4096 entries, a source the strips take."""
    rows, cols = case["H"].shape[:2]
    ih, iw = case["img"].shape[:2]
    fw, fh = case["final"][:2]
    strips = iw < 1 << 24 and ih < 1 << 24 and ih * iw * 3 < 1 << 31
    tables = len(case["mesh"][0]) <= 4096 and len(case["mesh"][1]) <= 4096 and rows < 65535 and cols < 65535
    return strips and tables and fw // cols <= FAST_MEAN_CELL and fh // rows <= FAST_MEAN_CELL


def _pad_axis(edges, count):
    """Edges 1 px apart appended beyond the last one until count // cells <= 128: cells that hold no canvas pixel, so the cells
    of 254 px stay as they are and the mesh's mean cell is small enough for the estimate kernel."""
    edges = [float(e) for e in edges]
    assert edges[-1] >= count
    while count // (len(edges) - 1) > FAST_MEAN_CELL:
        edges.append(edges[-1] + 1.0)
    return edges


def _finish(name, group, H, kinds, mesh_w, mesh_h, final, img_hw=None, center_hw=None, pad=True):
    fw, fh, ox, oy = final
    if pad:         # cells beyond the canvas edge: identity matrices that no pixel reads
        mesh_w, mesh_h = _pad_axis(mesh_w, fw), _pad_axis(mesh_h, fh)
        rows, cols = H.shape[:2]
        full = np.tile(np.eye(3, dtype=np.float32), (len(mesh_h) - 1, len(mesh_w) - 1, 1, 1))
        full[:rows, :cols] = H
        names = np.full(full.shape[:2], None, object)
        for rc in np.ndindex(names.shape):
            names[rc] = kinds[rc] if rc[0] < rows and rc[1] < cols else dict(kind="beyond the canvas", m=0, e=0, s=0)
        H, kinds = full, names
    H = np.ascontiguousarray(H, np.float32)
    mesh = (np.asarray(mesh_w, np.float64), np.asarray(mesh_h, np.float64))
    hinv = checked_inverse(H)
    tx, ty = O.warp_coords_fast(hinv, mesh, (fw, fh), (ox, oy))
    if img_hw is None:
        img_hw = (int(np.ceil(ty.max())) + 4, int(np.ceil(tx.max())) + 4)
    img = picture(*img_hw)
    rng = np.random.default_rng(sum(map(ord, name)))
    center = _center(rng, *center_hw) if center_hw else None
    if center is not None:
        assert 0 <= ox and ox + center.shape[1] <= fw and 0 <= oy and oy + center.shape[0] <= fh
    for a in (img, H, hinv, tx, ty, mesh[0], mesh[1]) + ((center,) if center is not None else ()):
        a.setflags(write=False)
    return dict(name=name, group=group, img=img, H=H, mesh=mesh, final=final, center=center, hinv=hinv, kinds=kinds, coords=(tx, ty))


E_ALL = (16, 17, 18, 19, 20, 21)
SWEEP_GEO = dict(mesh_w=[0.0, 254, 508, 762], mesh_h=[0.0, 254, 508], final=(762, 508, 3, 2), img_hw=(1530, 2290))


def _corner(mesh_w, mesh_h, r, c, final, lo=False):
    """Cell (r, c)'s far corner, three pixels inside it, relative to the offsets."""
    x = (mesh_w[c] + 3) if lo else (min(mesh_w[c + 1], mesh_w[c] + CELL) - 4)
    y = (mesh_h[r] + 3) if lo else (min(mesh_h[r + 1], mesh_h[r] + CELL) - 4)
    return x - final[2], y - final[3]


def _sweep(m, s):
    """One multiplier and one sign on the six exponents: 3 x 2 cells of 254 x 254.  All six such cases share mesh, canvas,
    offsets and picture, so they also go through one batched launch."""
    g = SWEEP_GEO
    H = np.empty((2, 3, 3, 3), np.float32)
    kinds = np.empty((2, 3), object)
    for k, e in enumerate(E_ALL):
        r, c = divmod(k, 3)
        H[r, c] = sweep_cell(m, e, s, _corner(g["mesh_w"], g["mesh_h"], r, c, g["final"]))
        kinds[r, c] = dict(kind="plain", m=m, e=e, s=s)
    return _finish(f"sweep_m{m}{'p' if s > 0 else 'n'}", "sweep", H, kinds, g["mesh_w"], g["mesh_h"], g["final"], g["img_hw"], (300, 400))


def _sweep_turned(name="sweep_turned", pad=True):
    """Row 0: quarter turns (u = 256 - y, v = x), the sweep of tx runs along dy.  Row 1: mild perspective (2^-13, -2^-14 in
    the forward matrix's third row) that the record still accepts.  Canvas width 4 k + 3.  ``pad=False``: the same cells on
    a mesh of 4 x 2 cells, whose mean cell of 253 px keeps the all-float64 strips whatever the context asks for."""
    mesh_w, mesh_h, final = [0.0, 254, 508, 762, 1016], [0.0, 254, 508], (1015, 508, 0, 0)
    H = np.empty((2, 4, 3, 3), np.float32)
    kinds = np.empty((2, 4), object)
    for c, (m, e, s) in enumerate(((1, 16, 1), (2, 18, -1), (1, 20, 1), (1, 21, -1))):
        H[0, c] = sweep_cell(m, e, s, _corner(mesh_w, mesh_h, 0, c, final, lo=(c % 2 == 1)), L=TURN, K=(256, 0))
        kinds[0, c] = dict(kind="turned", m=m, e=e, s=s)
    for c, (m, e, s) in enumerate(((1, 16, -1), (1, 18, 1), (1, 19, -1), (1, 21, 1))):
        H[1, c] = sweep_cell(m, e, s, _corner(mesh_w, mesh_h, 1, c, final), persp=(2.0 ** -13, -2.0 ** -14))
        kinds[1, c] = dict(kind="perspective", m=m, e=e, s=s)
    return _finish(name, "sweep" if pad else "coarse", H, kinds, mesh_w, mesh_h, final, None, (200, 300), pad=pad)


def _cap():
    """Magnification 3 (1 +- 2^-e) under the shear u = x + y on cells 254 and 200 px wide and 100 high: the record's bound of
    |estimate| is 3 (127 + 50) = 531 px on the wide cells - above kFastMaxEstimate = 500, every pixel takes the exact path -
    and 3 (100 + 50) = 450 px on the others, which keep a bound with a wide window.  Canvas width 4 k + 1, a negative offset."""
    mesh_w, mesh_h, final = [0.0, 254, 454, 708, 908], [0.0, 100, 200, 300], (905, 300, -5, 4)
    H = np.empty((3, 4, 3, 3), np.float32)
    kinds = np.empty((3, 4), object)
    for k in range(12):
        r, c = divmod(k, 4)
        e, s = E_ALL[k % 6], (1 if (k // 2) % 2 == 0 else -1)
        H[r, c] = sweep_cell(3, e, s, _corner(mesh_w, mesh_h, r, c, final), L=SHEAR, mid=round(1.2 * BAND_MID * 2.0 ** e))
        kinds[r, c] = dict(kind="cap", m=3, e=e, s=s)
    return _finish("cap", "cap", H, kinds, mesh_w, mesh_h, final)


def _wide():
    """Cell columns of 254, 255, 256, 2 and 249 px: pixels past the clamped span of 254 go to the extra column (everything in
    doubt), and the 2 px column (canvas columns 765, 766) puts a third cell inside a lane's group of four.  Canvas width
    4 k + 1, a negative offset."""
    mesh_w, mesh_h, final = [0.0, 254, 509, 765, 767, 1016], [0.0, 254, 508], (1013, 508, 0, -6)
    H = np.empty((2, 5, 3, 3), np.float32)
    kinds = np.empty((2, 5), object)
    for r, s in enumerate((1, -1)):
        for c, e in enumerate((16, 18, 20, 17, 21)):
            H[r, c] = sweep_cell(1, e, s, _corner(mesh_w, mesh_h, r, c, final))
            kinds[r, c] = dict(kind="wide", m=1, e=e, s=s)
    return _finish("wide", "wide", H, kinds, mesh_w, mesh_h, final)


INT_IMG = (230, 240)        # (h, w) of the integer cases' picture: both borders fall inside every 254 px cell


def _integers(name, final, first):
    """Integer translations, each through a common factor (one cell column each: 7, 1, 3, 5): every coordinate is an exact
    integer and, but for the factor 1, the quotient of a real division whose divisor is no power of two.  Every cell's first
    canvas pixel maps to about ``first``, so its columns and rows run through t = 0 and t = size (outside by the strict test)
    and their inside neighbours 1 and size - 1.  No float32 p has fl32(1 / p) = 7 (the reciprocals of the float32 next to 1 / 7
    lie 1.5 ulp of 7 apart), so that column is fl32(1 / 7) [[1, 0, -A], [0, 1, -B], [0, 0, 1]] with A, B powers of two: its
    inverse is 7 - 2^-21 times the integer translation, every entry exact."""
    mesh_w, mesh_h = [0.0, 254, 508, 762, 1016], [0.0, 254, 508]
    H = np.empty((2, 4, 3, 3), np.float32)
    kinds = np.empty((2, 4), object)
    pow2 = lambda t: 0.0 if t == 0 else float(np.sign(t)) * 2.0 ** round(np.log2(abs(t)))       # noqa: E731
    for r in range(2):
        for c, f in enumerate((7, 1, 3, 5)):
            x0, y0 = mesh_w[c] - final[2], mesh_h[r] - final[3]
            if f == 7:
                A, B = pow2(first[0] - x0), pow2(first[1] - y0)
                p = np.float32(1.0 / 7.0)
                M = (np.array([[1, 0, -A], [0, 1, -B], [0, 0, 1]], np.float64) * float(p)).astype(np.float32)
                f = float(_round_f32(1 / Fraction(float(p))))
                assert f == 7.0 - 2.0 ** -21
            else:
                for d in (0, 1, -1, 2, -2, 3, -3, 4, -4):       # a start for which the factor has a float32 forward matrix
                    A, B = first[0] + d - x0, first[1] - d - y0
                    M = integer_cell(f, A, B)
                    if M is not None:
                        break
            assert M is not None, (r, c, f)
            H[r, c] = M
            kinds[r, c] = dict(kind="integer", m=1, factor=f, A=A, B=B)
    case = _finish(name, "integers", H, kinds, mesh_w, mesh_h, final, INT_IMG, (120, 200))
    for r in range(2):
        for c in range(4):
            k = kinds[r, c]
            want = np.array([[1, 0, k["A"]], [0, 1, k["B"]], [0, 0, 1]], np.float64) * k["factor"]
            assert np.array_equal(case["hinv"][r, c].astype(np.float64), want), (r, c)
    return case


def _f64():
    """Float64 grids for ``APAP.local_warp``: scales 1 +- 2^-e, e = 40 .. 46, all divided by 3 (the third component of the
    inverse is 3: a real division), which leave the coordinates within 2^-36 of integers on either side, and two cells with
    an integer translation and third component 3.  4 x 4 cells of 127 x 64 px."""
    mesh_w, mesh_h, final = np.linspace(0.0, 508.0, 5), np.linspace(0.0, 256.0, 5), (508, 256, 0, 0)
    H = np.empty((4, 4, 3, 3), np.float64)
    kinds = np.empty((4, 4), object)
    for k in range(16):
        r, c = divmod(k, 4)
        if k < 14:
            e, s = 40 + k // 2, (1 if k % 2 == 0 else -1)
            sc = 1.0 + s * 2.0 ** -e
            H[r, c] = np.array([[sc, 0, -3.0], [0, sc, -2.0], [0, 0, 1.0]]) / 3.0
            kinds[r, c] = dict(kind="f64", e=e, s=s)
        else:
            H[r, c] = np.array([[1.0, 0, -3.0], [0, 1.0, -2.0], [0, 0, 1.0]]) / 3.0
            kinds[r, c] = dict(kind="f64 integer")
    img = picture(270, 520)
    for a in (img, H, mesh_w, mesh_h):
        a.setflags(write=False)
    return dict(name="f64", group="f64", img=img, H=H, mesh=(mesh_w, mesh_h), final=final, center=None, kinds=kinds)


_BUILDERS = {f"sweep_m{m}{t}": (lambda m=m, s=s: _sweep(m, s)) for m in (1, 2, 3) for t, s in (("p", 1), ("n", -1))}
_BUILDERS.update(sweep_turned=_sweep_turned, cap=_cap, wide=_wide, coarse=lambda: _sweep_turned("coarse", pad=False),
                 integers_a=lambda: _integers("integers_a", (1016, 508, 4, 6), (-7, -5)),
                 integers_b=lambda: _integers("integers_b", (1014, 507, 0, 0), (-2, -9)))
BATCH_CASES = tuple(f"sweep_m{m}{t}" for m in (1, 2, 3) for t in "pn")       # one geometry, one picture
FAST_CASES = BATCH_CASES + ("sweep_turned", "cap", "wide", "integers_a", "integers_b")     # the estimate kernel's
F32_CASES = FAST_CASES + ("coarse",)        # and sweep_turned's cells on a mesh that keeps the all-float64 strips
STITCH_CASES = tuple(n for n in F32_CASES if n.startswith(("sweep", "integers", "coarse")))
EDGE_CASES = tuple(n for n in FAST_CASES if not n.startswith("integers"))     # sweep + cap + wide


def get(name):
    if name not in _cases:
        _cases[name] = _f64() if name == "f64" else _BUILDERS[name]()
    return _cases[name]


def classify(name, rcp_ulps=0):
    """Every canvas pixel of a float32 case through the restated set-up tables (``S.origin``, ``S.record``), the kernel's
    float32 arithmetic (``S.estimate``) and the reference's coordinates on the designed inverse.  Returns a dict of
    (fh, fw) arrays: ``doubt`` (flagged, pixels outside an ordinary cell's clamped span included), ``ix, iy`` (the estimate's
    integers), ``tx, ty``, ``win`` (the cell's window in px, inf without a bound), ``above`` / ``below`` (near misses: not
    flagged, tx or ty within two windows above / below an integer), ``far`` (|dx|, |dy| >= 120), ``integer`` (tx or ty is an
    integer), ``good`` (the pixel's cell keeps a bound), ``cr, cc`` (cell row and column)."""
    key = (name, rcp_ulps if isinstance(rcp_ulps, int) else "mixed")
    if key in _classes:
        return _classes[key]
    case = get(name)
    fw, fh, ox, oy = case["final"]
    mesh_w, mesh_h = case["mesh"]
    rows, cols = case["H"].shape[:2]
    hinv = case["hinv"].astype(np.float64).reshape(rows, cols, 9)
    okx, x0, sx = S.origin(mesh_w, fw)
    oky, y0, sy = S.origin(mesh_h, fh)
    rec = S.record(hinv, oky[:, None] & okx[None, :], (x0 + sx // 2 - ox)[None, :].astype(float), (y0 + sy // 2 - oy)[:, None].astype(float),
                   (sx - sx // 2)[None, :].astype(float), (sy - sy // 2)[:, None].astype(float))
    jj, ii = np.arange(fw), np.arange(fh)
    cc, cr = O.cell_lookup(fw, mesh_w), O.cell_lookup(fh, mesh_h)
    inx = okx[cc] & (jj - x0[cc] >= 0) & (jj - x0[cc] < sx[cc])
    iny = oky[cr] & (ii - y0[cr] >= 0) & (ii - y0[cr] < sy[cr])
    inside = iny[:, None] & inx[None, :]                    # else the extra row / column: everything in doubt
    dx = np.where(inx, jj - x0[cc] - sx[cc] // 2, 0)[None, :]
    dy = np.where(iny, ii - y0[cr] - sy[cr] // 2, 0)[:, None]
    cell = {k: v[cr[:, None], cc[None, :]] for k, v in rec.items()}
    ix, iy, doubt = S.estimate(cell, dx, dy, rcp_ulps)
    doubt = doubt | ~inside
    tx, ty = case["coords"]
    win = np.where(cell["good"], cell["thr"] / S.UNIT, np.inf)
    sure = ~doubt
    up = np.minimum(tx - np.floor(tx), ty - np.floor(ty))
    down = np.minimum(np.ceil(tx) - tx, np.ceil(ty) - ty)
    integer = (tx == np.floor(tx)) | (ty == np.floor(ty))
    out = dict(doubt=doubt, ix=ix, iy=iy, tx=tx, ty=ty, win=win, above=sure & (up < 2 * win), below=sure & (down < 2 * win),
               far=(np.abs(dx) >= FAR) & (np.abs(dy) >= FAR) & inside, integer=integer, good=cell["good"] & inside,
               cr=np.broadcast_to(cr[:, None], (fh, fw)), cc=np.broadcast_to(cc[None, :], (fh, fw)))
    if isinstance(rcp_ulps, int):
        _classes[key] = out
    return out


def describe(name, got, want):
    """Where a canvas differs from the oracle's, by the classes of the differing pixels (for an assertion's message)."""
    bad = (got != want).any(axis=-1)
    if not bad.any():
        return ""
    k = classify(name)
    y, x = np.argwhere(bad)[0]
    kinds = get(name)["kinds"]
    cells = sorted({(int(r), int(c)) for r, c in zip(k["cr"][bad], k["cc"][bad])})
    return (f"{name}: {int(bad.sum())} pixels differ; first at (y, x) = ({y}, {x}): {got[y, x]} != {want[y, x]}, t = ({k['tx'][y, x]!r}, "
            f"{k['ty'][y, x]!r}); flagged {int((bad & k['doubt']).sum())}, near misses above {int((bad & k['above']).sum())}, below "
            f"{int((bad & k['below']).sum())}, exact integers {int((bad & k['integer']).sum())}; cells "
            + ", ".join(f"{rc}: {kinds[rc]}" for rc in cells[:6]))
