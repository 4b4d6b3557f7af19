"""What the two matchers share, without a GPU: the one split rule against both earlier formulas, the workspace sizes against
recorded values, and the specification's single-rounding fmaf against libm's."""
import ctypes as C

import numpy as np

import match_spec as S

# 1, each query tile (64, 256) and the train chunk (128) minus and plus one, 5000, the most rows of a pair
SIZES = (1, 63, 65, 127, 129, 255, 257, 5000, 1 << 24)

# apap_match_batch_workspace_bytes / apap_match_guided_batch_workspace_bytes of one pair, {nq: values over nt in SIZES}, as
# the library returned them before the two sources shared plan_split
MATCH = {
    1: (512, 512, 512, 512, 512, 512, 512, 1024, 65792),
    63: (1280, 1280, 1280, 1280, 2304, 2304, 3328, 40704, 4129024),
    65: (1536, 1536, 1536, 1536, 2560, 2560, 3584, 41984, 2130176),
    127: (2304, 2304, 2304, 2304, 4352, 4352, 6400, 81664, 4161792),
    129: (2560, 2560, 2560, 2560, 4608, 4608, 6656, 82944, 2819840),
    255: (4352, 4352, 4352, 4352, 8448, 8448, 12544, 163584, 4178176),
    257: (4608, 4608, 4608, 4608, 8704, 8704, 12800, 164864, 3372288),
    5000: (80384, 80384, 80384, 80384, 160256, 160256, 240384, 3200256, 4160256),
    16777216: (268435712, 268435712, 268435712, 268435712, 268435712, 268435712, 268435712, 268435712, 268435712),
}
GUIDED = {
    1: (768, 1024, 1280, 1536, 1792, 2560, 2816, 41472, 134242560),
    63: (2048, 2304, 2560, 2816, 4608, 5376, 7168, 101120, 135766272),
    65: (2304, 2560, 2816, 3072, 4864, 5632, 7424, 102912, 135815424),
    127: (3584, 3840, 4096, 4352, 7680, 8448, 11776, 162560, 137339136),
    129: (3840, 4096, 4352, 4608, 7936, 8704, 12032, 164352, 137388288),
    255: (6656, 6912, 7168, 7424, 13824, 14592, 20992, 285440, 140484864),
    257: (6912, 7168, 7424, 7680, 14080, 14848, 21248, 287232, 137376000),
    5000: (120576, 120832, 121088, 121344, 241664, 242432, 362752, 4840448, 140457984),
    16777216: (402653696, 402653952, 402654208, 402654464, 402654720, 402655488, 402655744, 402693632, 536871168),
}
# ... and of the 64 pairs of SIZES without the last in one batch (nq-major), the offsets starting at 3 and 5
MATCH_BATCH, GUIDED_BATCH = 4823552, 7598848


def p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def test_train_splits_equals_both_earlier_formulas(native):
    assert (native.MATCH_QUERY_TILE, native.MATCH_TRAIN_CHUNK, native.GUIDED_QUERY_TILE, native.GUIDED_TRAIN_CHUNK) == (64, 128, 256, 128)
    for nq in SIZES:
        for nt in SIZES:
            # match_splits, as it was
            q_tiles = -(-int(nq) // 64)
            chunks = -(-int(nt) // 128)
            per = -(-chunks // min(chunks, -(-4096 // q_tiles)))
            assert native.match_splits(nq, nt) == native.train_splits(nq, nt, 64, 128, 4096) == (-(-chunks // per), per), (nq, nt)
            # guided_splits, as it was
            q_tiles = -(-int(nq) // 256)
            chunks = -(-int(nt) // 128)
            per = -(-chunks // min(chunks, -(-1024 // q_tiles)))
            assert native.guided_splits(nq, nt) == native.train_splits(nq, nt, 256, 128, 1024) == (-(-chunks // per), per), (nq, nt)


def test_workspace_sizes_are_the_recorded_ones(native):
    lib = native.lib()
    for nq in SIZES:
        for k, nt in enumerate(SIZES):
            qo, to = np.array([0, nq], np.int32), np.array([0, nt], np.int32)
            assert lib.apap_match_batch_workspace_bytes(p(qo), p(to), 1) == lib.apap_match_workspace_bytes(nq, nt) == MATCH[nq][k], (nq, nt)
            assert lib.apap_match_guided_batch_workspace_bytes(p(qo), p(to), 1) == lib.apap_match_guided_workspace_bytes(nq, nt) \
                == GUIDED[nq][k], (nq, nt)
    ql, tl = [a for a in SIZES[:-1] for b in SIZES[:-1]], [b for a in SIZES[:-1] for b in SIZES[:-1]]
    qo, to = np.cumsum([3] + ql).astype(np.int32), np.cumsum([5] + tl).astype(np.int32)
    assert lib.apap_match_batch_workspace_bytes(p(qo), p(to), len(ql)) == MATCH_BATCH
    assert lib.apap_match_guided_batch_workspace_bytes(p(qo), p(to), len(ql)) == GUIDED_BATCH


def fma_triples():
    """A few thousand (a, b, c) float32: random at mixed scales; a * b + c exactly in the middle of two float32 and one float32
    step of c off it; and a * b itself in the middle with a c far below the last bit of a float64 sum - where a plain float64
    add loses c and the cast goes to even."""
    rng = np.random.default_rng(41)
    f32 = np.float32
    a = (rng.normal(0, 1, 3000) * 2.0 ** rng.integers(-20, 20, 3000)).astype(f32)
    b = (rng.normal(0, 1, 3000) * 2.0 ** rng.integers(-20, 20, 3000)).astype(f32)
    c = (rng.normal(0, 1, 3000) * 2.0 ** rng.integers(-40, 40, 3000)).astype(f32)
    out = [(a, b, c), (a[:500], b[:500], (-(a[:500].astype(np.float64) * b[:500])).astype(f32))]      # cancellation
    # the middle: lo < p < hi neighbouring float32, c = (lo + hi) / 2 - p where that is a float32 (it mostly is: 24 bits)
    x, y = rng.uniform(1, 2, 1000).astype(f32), rng.uniform(1, 2, 1000).astype(f32)
    prod = x.astype(np.float64) * y
    near = prod.astype(f32)
    lo = np.where(near > prod, np.nextafter(near, f32(0)), near).astype(f32)
    mid = (lo.astype(np.float64) + np.nextafter(lo, f32(4)).astype(np.float64)) / 2
    c0 = (mid - prod).astype(f32)
    tie = c0.astype(np.float64) == mid - prod
    assert tie.sum() > 500
    x, y, c0 = x[tie], y[tie], c0[tie]
    out += [(x, y, c0), (x, y, np.nextafter(c0, f32(1))), (x, y, np.nextafter(c0, f32(-1)))]
    # (1 + 2^-i)(1 + 2^-(24 - i)) = 1 + 2^-i + 2^-(24 - i) + 2^-24: 25 bits, the middle of two float32
    i = np.arange(1, 24)
    x, y = (1 + 2.0 ** -i).astype(f32), (1 + 2.0 ** -(24.0 - i)).astype(f32)
    for scale in (1.0, 2.0 ** 10, -(2.0 ** -30)):
        for tiny in (0.0, 2.0 ** -60, -(2.0 ** -60), 2.0 ** -100, -(2.0 ** -100)):
            out.append((x * f32(scale), y, np.full(len(i), tiny * abs(scale), f32)))
    return tuple(np.concatenate(v) for v in zip(*out))


def test_the_specifications_fmaf_equals_libms():
    libm = C.CDLL("libm.so.6")
    libm.fmaf.restype = C.c_float
    libm.fmaf.argtypes = [C.c_float] * 3
    a, b, c = fma_triples()
    assert len(a) > 4000
    want = np.array([libm.fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], np.float32)
    got = S.fmaf(a, b, c)
    assert got.tobytes() == want.tobytes(), int(np.count_nonzero(got.view(np.int32) != want.view(np.int32)))
    # the triples bite: a float64 multiply and add, cast to float32, is wrong on some of them
    plain = (a.astype(np.float64) * b + c).astype(np.float32)
    assert np.count_nonzero(plain.view(np.int32) != want.view(np.int32)) >= 20
