"""Inputs that reach the edges of the kernels of csrc/apap_frontend.hip - per-channel histogram equalisation and the RANSAC
seed homography - which seeded random shapes do not: test infrastructure shared by tests/test_frontend_edge_inputs.py, which
asserts from oracle/frontend_oracle.py alone that every input reaches its edge, and tests/test_gpu_frontend_edges.py, which
runs them on the GPU.  numpy only.  The constants named here are those of csrc/apap_frontend.hip."""
import numpy as np

import test_frontend as TF
from oracle import frontend_oracle as F

# ---------------------------------------------------------------- equalisation
CHUNK = 3072                 # kEqChunkVecs * 16: the bytes a wave streams per step, a multiple of every channel count
MAX_BLOCKS, WAVES = 1024, 4  # the capped grid of launch_equalize: 4096 waves, a wave loops only above 4096 chunks
REPLICAS = 16                # kEqReplicas: the workspace starts with REPLICAS x C x 256 uint32 counters
HEAD_OFFSETS = (0, 1, 2, 3, 5, 15)
BIN_FIRSTS = (0, 63, 64, 127, 128, 191, 192, 254)   # either side of the table builder's four waves of 64 bins


def eq_split(offset, nbytes):
    """(head, chunks, tail bytes) of eq_split for an image of ``nbytes`` bytes that starts ``offset`` bytes after a 16-byte
    boundary: the bytes before the first boundary, the whole chunks of the aligned body, and what is left."""
    head = min(nbytes, (16 - offset % 16) % 16)
    chunks = (nbytes - head) // CHUNK
    return head, chunks, nbytes - head - chunks * CHUNK


def other_offset(off_in):
    """An output offset whose body is not 16-byte aligned when the input's is: the unaligned dword stores of k_eq_apply."""
    return (off_in + 3) % 16


def eq_tails(C, off_in):
    """The three tail lengths in bytes for an image of C-byte pixels behind a head of (16 - off_in) % 16 bytes: the fewest the
    pixel size allows (none when the head is whole pixels, else the rest of the pixel the head cut), one pixel more, and one
    pixel short of a further chunk."""
    head = (16 - off_in % 16) % 16
    t0 = -head % C
    return t0, t0 + C, t0 + C * ((CHUNK - 1 - t0) // C)


def eq_sizes(C, off_in=0):
    """Shapes (1, w, C) that put exactly 0, 1 and 2 chunks in the aligned body behind the head of ``off_in``, each with the
    three tails of ``eq_tails``; the empty image is left out."""
    head = (16 - off_in % 16) % 16
    out = []
    for chunks in (0, 1, 2):
        for tail in eq_tails(C, off_in):
            nbytes = head + chunks * CHUNK + tail
            assert nbytes % C == 0
            if nbytes:
                out.append((1, nbytes // C, C))
    return out


def eq_tiny():
    """(shape, input offset) of images that end before the first 16-byte boundary (or on it): the min(bytes, ...) of
    eq_split, no body and no tail."""
    return [((1, 1, 3), 1), ((1, 1, 1), 15), ((1, 1, 1), 3), ((1, 2, 2), 5), ((1, 3, 4), 2), ((1, 1, 4), 5), ((2, 2, 3), 3),
            ((1, 5, 3), 1)]


def eq_image(shape, seed=0):
    """Narrow bands that differ per channel (large bins, another table for every channel: a byte read with the wrong channel
    phase maps wrongly), every 7th pixel anywhere in 0 .. 255."""
    rng = np.random.default_rng([seed, *shape])
    h, w, C = shape
    img = (rng.integers(0, 256, shape) >> 3) + 40 + 37 * np.arange(C)
    wide = rng.integers(0, 256, shape)
    pick = (np.arange(h * w).reshape(h, w, 1) % 7) == 3
    return np.where(pick, wide, img).astype(np.uint8)


def _plane(levels, shape, rng):
    """A plane of ``shape`` that holds every one of ``levels`` and nothing else, with unequal counts."""
    levels = np.asarray(levels, dtype=np.uint8)
    size = shape[0] * shape[1]
    assert size >= 2 * len(levels)
    weights = rng.random(len(levels)) ** 3 + 1e-3
    rest = rng.choice(levels, size - len(levels), p=weights / weights.sum())
    return rng.permutation(np.concatenate([levels, rest])).reshape(shape)


def eq_bins(kind, shape=(23, 57)):
    """First occupied grey level -> plane.  ``"above"``: every level from the first up to 255 is occupied; ``"two"``: only
    the first level and 255; ``"all"``: all 256 levels (first level 0 only).  The first levels sit on either side of the
    64-bin waves of eq_build_luts, whose ballots find the first bin and whose scan covers the bins after it."""
    rng = np.random.default_rng(len(kind))
    if kind == "all":
        return {0: _plane(np.arange(256), shape, rng)}
    assert kind in ("above", "two")
    return {i0: _plane(np.arange(i0, 256) if kind == "above" else [i0, 255], shape, rng) for i0 in BIN_FIRSTS}


def eq_four_channels(shape=(19, 45)):
    """4 channels: constant at 255, two levels (100 and 200), first bin 64, first bin 191.  The table is built for all four at
    once, so one channel's first bin, count or sums must not reach another's."""
    rng = np.random.default_rng(4)
    planes = [np.full(shape, 255, np.uint8), _plane([100, 200], shape, rng), _plane(np.arange(64, 256, 3), shape, rng),
              _plane(np.arange(191, 256), shape, rng)]
    return np.ascontiguousarray(np.stack(planes, -1))


def eq_known_answers():
    """(plane, answer) with the answer written out by hand: cvRound's ties to even (scale 255 / 6: the running sum 1 gives
    42.5 -> 42, 3 gives 127.5 -> 128) and two levels 3 : 1."""
    return [(np.array([[0, 1, 2, 2, 3, 4, 4]], np.uint8), np.array([[0, 42, 128, 128, 170, 255, 255]], np.uint8)),
            (np.array([[10, 10, 10, 200]], np.uint8), np.array([[0, 0, 0, 255]], np.uint8))]


STRIDED_SHAPES = {1: (6144, 3072, 1), 2: (3072, 3072, 2), 4: (1536, 3072, 4)}


def eq_strided(C):
    """18.9 MB, 6144 chunks when aligned: of the 4096 waves of the capped grid the first 2048 take a second chunk, the others
    do not - the smallest size at which the register double buffer carries a chunk over.  Narrow bands per channel."""
    rng = np.random.default_rng(60 + C)
    img = rng.integers(0, 256, STRIDED_SHAPES[C], dtype=np.uint8)
    img >>= 3
    img += (40 + 37 * np.arange(C)).astype(np.uint8)
    return img


# ---------------------------------------------------------------- RANSAC
# a case is (src, dst, thresh, iterations, seed): the arguments of F.ransac_core and of apap_ransac_device
HYP_LANES, SCORE_THREADS = 64, 256      # kHypLanes; the block of k_ransac_score and k_ransac_select
GRID_K = (1, 63, 64, 65, 255, 256, 257, 2049)
GRID_N = (5, 6, 7, 255, 256, 257, 513)
SEEDS = (0, (1 << 64) - 5, 1 << 63)
THRESHOLDS = (0.0, 1e-200, 1e200)       # the squares of the last two are 0 and inf


def ransac_noisy(n, K, seed=F.RANSAC_SEED, thresh=5.0):
    """The noisy scene of test_frontend.ransac_case, 25 % outliers."""
    src, dst, _, _ = TF.ransac_case(n, 0.25, seed=n)
    return src, dst, thresh, K, seed


def ransac_ties(seed=2, n=257, K=600, n_out=40):
    """Integer points on the exact similarity dst = 2 src + t, with planted integer outliers: every hypothesis drawn from
    four good points is the similarity up to rounding and counts all n - n_out of them, so hundreds of hypotheses tie at the
    maximum.  n = 257 puts one point in the second trip of the 256-thread scoring loop, K = 600 three hypotheses in some
    threads of the selection and two in others."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 1000, (n, 2)).astype(np.float32)
    dst = 2 * src + np.array([30, -20], np.float32)
    bad = rng.choice(n, n_out, replace=False)
    dst[bad] = rng.integers(0, 2000, (n_out, 2)).astype(np.float32)
    return src, dst, 5.0, K, F.RANSAC_SEED


def tie_facts(counts):
    """What the tie case must show, from the K inlier counts: the tied indices, the first, the tied g > first in a selection
    thread before the first one's, the i with i and i + 256 both tied."""
    tied = np.flatnonzero(counts == counts.max())
    first = int(tied[0])
    earlier_thread = [int(g) for g in tied if g > first and g % SCORE_THREADS < first % SCORE_THREADS]
    same_thread = [int(i) for i in tied if i + SCORE_THREADS in set(tied.tolist())]
    return dict(tied=tied, first=first, earlier_thread=earlier_thread, same_thread=same_thread)


def ransac_all_nan(K=128):
    """Nine copies of one source point: after the first elimination step the second column of every 8 x 8 system is exactly
    zero (the multipliers are exactly 1), so every hypothesis is NaN, nothing is an inlier and the winner is hypothesis 0."""
    rng = np.random.default_rng(9)
    src = np.tile(np.array([[3, 5]], np.float32), (9, 1))
    dst = (rng.random((9, 2)) * 100).astype(np.float32)
    return src, dst, 5.0, K, F.RANSAC_SEED


def ransac_duplicates():
    """Every correspondence twice, n = 60: a sample that draws both copies of one has two equal pairs of rows and an exactly
    zero pivot - NaN rows among finite ones."""
    src, dst, _, _ = TF.ransac_case(30, 0.2, seed=30)
    return np.repeat(src, 2, axis=0), np.repeat(dst, 2, axis=0), 5.0, 512, F.RANSAC_SEED


COUNT_CASES = {4: (0, 1e-6), 3: (15, 0.0)}      # best count -> (scene seed, threshold), found by searching scene seeds


def ransac_count(k):
    """40 unrelated random points and a tiny threshold: the best of 256 hypotheses keeps only its own sample (k = 4) or, at
    threshold 0, the 3 points of it that it reproduces without any rounding error (k = 3)."""
    scene, thresh = COUNT_CASES[k]
    rng = np.random.default_rng(scene)
    src = (rng.random((40, 2)) * 1000).astype(np.float32)
    dst = (rng.random((40, 2)) * 1000).astype(np.float32)
    return src, dst, thresh, 256, F.RANSAC_SEED


_cases, _cores = {}, {}


def ransac_cases():
    """Name -> case, everything that is compared with the oracle hypothesis by hypothesis (built once)."""
    if not _cases:
        _cases.update(_build_cases())
    return _cases


def _build_cases():
    cases = {"ties": ransac_ties(), "all NaN": ransac_all_nan(), "duplicates": ransac_duplicates(),
             "count 3": ransac_count(3), "count 4": ransac_count(4)}
    for K in GRID_K:
        cases[f"n=57 K={K}"] = ransac_noisy(57, K)
    for n in GRID_N:
        cases[f"n={n} K=65"] = ransac_noisy(n, 65)
    for seed in SEEDS:
        cases[f"seed {seed:#x}"] = ransac_noisy(57, 65, seed=seed)
    for thresh in THRESHOLDS:
        cases[f"thresh {thresh:g}"] = ransac_noisy(57, 65, thresh=thresh)
        cases[f"duplicates, thresh {thresh:g}"] = ransac_duplicates()[:2] + (thresh, 512, F.RANSAC_SEED)
    return cases


def ransac_core(name):
    """The oracle's answer for a case of ``ransac_cases``, computed once."""
    if name not in _cores:
        _cores[name] = F.ransac_core(*ransac_cases()[name])
    return _cores[name]


# ---------------------------------------------------------------- the sampler's smallest pools
# The sampler is one template (csrc/apap_ransac_dev.h) at 4 draws (homography) and at 8 (fundamental matrix).  Its smallest
# pools: n = K, where the last draw is taken modulo 1 and every pick is forced by the step-over, and n = K + 1; 65
# iterations, so that the second block of hypotheses has one live lane; the default seed and one whose counter wraps.
POOL_ITERATIONS = 65
POOL_SEEDS = {"default": None, "wrap": (1 << 64) - 5}
SMALL_POOLS = [("homography", 4), ("homography", 5), ("fundamental", 8), ("fundamental", 9)]


def small_pool_case(model, n, seed_name):
    """A clean scene of n matches: a ``ransac_cases`` tuple for the homography, a ``fundamental_cases.Case`` for the
    fundamental matrix (its specification's default seed is its own)."""
    seed = POOL_SEEDS[seed_name]
    if model == "homography":
        src, dst, _, _ = TF.ransac_case(n, 0.0, seed=n)
        return src, dst, 5.0, POOL_ITERATIONS, F.RANSAC_SEED if seed is None else seed
    import fundamental_cases as C
    s = C.two_pose_scene(n, 300 + n, noise=0.5)
    settings = {} if seed is None else {"seed": seed}
    return C.Case(f"pool n{n} {seed_name}", s.src, s.dst, 3.0, POOL_ITERATIONS, **settings)


def small_pool_core(model, n, seed_name):
    """The specification's answer for ``small_pool_case``, computed once."""
    key = (model, n, seed_name)
    if key not in _cores:
        case = small_pool_case(model, n, seed_name)
        if model == "homography":
            _cores[key] = F.ransac_core(*case)
        else:
            import fundamental_cases as C
            _cores[key] = C.expected(case)
    return _cores[key]
