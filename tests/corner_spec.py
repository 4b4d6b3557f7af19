"""The corner detector's contract (include/apap_hip.h "corner detection", DESIGN.md "Corner detection") in numpy int64: plain
array code, padded index arrays for reflect-101, an explicit loop over the window offsets.  No float anywhere."""
import numpy as np

I64_MIN = np.iinfo(np.int64).min


def grey(img):
    """(h, w) uint8 as it is; (h, w, 3) BGR -> (3735 B + 19235 G + 9798 R + 16384) >> 15, as int64."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    if img.ndim == 2 or img.shape[2] == 1:
        return img.reshape(img.shape[:2]).astype(np.int64)
    b, g, r = (img[:, :, k].astype(np.int64) for k in range(3))
    return (3735 * b + 19235 * g + 9798 * r + 16384) >> 15


def reflect101(n, pad=1):
    """Indices -pad .. n - 1 + pad reflected into 0 .. n - 1 without repeating the border (pad < n)."""
    i = np.arange(-pad, n + pad)
    i = np.abs(i)
    return np.where(i > n - 1, 2 * (n - 1) - i, i)


def padded(a):
    """`a` with one reflected row and column on every side: padded(a)[1 + y + dy, 1 + x + dx] is a[y + dy, x + dx] reflected."""
    return a[reflect101(a.shape[0])][:, reflect101(a.shape[1])]


def gradients(g):
    h, w = g.shape
    p = padded(g)
    at = lambda dy, dx: p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]     # noqa: E731
    ix = (at(-1, 1) + 2 * at(0, 1) + at(1, 1)) - (at(-1, -1) + 2 * at(0, -1) + at(1, -1))
    iy = (at(1, -1) + 2 * at(1, 0) + at(1, 1)) - (at(-1, -1) + 2 * at(-1, 0) + at(-1, 1))
    return ix, iy


def box3(a):
    h, w = a.shape
    p = padded(a)
    out = np.zeros_like(a)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            out += p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return out


def response(img):
    """R = 25 (a c - b^2) - (a + c)^2, int64 (h, w)."""
    ix, iy = gradients(grey(img))
    assert np.abs(ix).max() <= 1020 and np.abs(iy).max() <= 1020
    a, b, c = box3(ix * ix), box3(ix * iy), box3(iy * iy)
    assert max(a.max(), c.max(), np.abs(b).max()) <= 9 * 1020 ** 2
    R = 25 * (a * c - b * b) - (a + c) ** 2
    assert R.dtype == np.int64
    return R


def corner_mask(R, radius):
    """R > 0 and (R, -index) greater than every other pixel's of the window that lies inside the image."""
    h, w = R.shape
    big = np.full((h + 2 * radius, w + 2 * radius), I64_MIN, np.int64)
    big[radius:radius + h, radius:radius + w] = R
    ok = R > 0
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if dy == 0 and dx == 0:
                continue
            q = big[radius + dy:radius + dy + h, radius + dx:radius + dx + w]
            earlier = dy < 0 or (dy == 0 and dx < 0)          # q's index is the smaller one: it wins an equal response
            ok &= (q < R) if earlier else (q <= R)
    return ok


def bound(h, w, radius):
    s = radius + 1
    return -(-h // s) * -(-w // s)


def detect_full(img, max_corners, radius=5, quality_permille=10):
    """(pts (max_corners, 2) float32, response (max_corners,) int64, count): the library's outputs, rows from count on zero."""
    R = response(img)
    h, w = R.shape
    yy, xx = np.nonzero(corner_mask(R, radius))
    r = R[yy, xx]
    idx = yy * w + xx
    if len(r):
        keep = 1000 * r >= quality_permille * r.max()
        r, idx = r[keep], idx[keep]
    order = np.lexsort((idx, -r))[:max_corners]
    r, idx = r[order], idx[order]
    pts = np.zeros((max_corners, 2), np.float32)
    resp = np.zeros(max_corners, np.int64)
    pts[:len(r), 0], pts[:len(r), 1] = idx % w, idx // w
    resp[:len(r)] = r
    return pts, resp, len(r)


def detect(img, max_corners, radius=5, quality_permille=10):
    """(pts, response) trimmed to the count."""
    pts, resp, n = detect_full(img, max_corners, radius, quality_permille)
    return pts[:n], resp[:n]


def prototype_scene(h=200, w=260, seed=0, rects=30):
    """Box-blurred noise with flat rectangles: corners of every strength, and flat regions where R is 0 on a plateau."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, (h + 4, w + 4)).astype(np.int64)
    g = sum(g[dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5)) // 25
    for _ in range(rects):
        y, x = int(rng.integers(0, h - 8)), int(rng.integers(0, w - 8))
        hh, ww = int(rng.integers(6, 40)), int(rng.integers(6, 40))
        g[y:y + hh, x:x + ww] = int(rng.integers(0, 256))
    return g.astype(np.uint8)
