"""Inputs for the ORB stage tests (tests/test_orb_stages_cpu.py, tests/test_orb_stages_gpu.py): numpy only, every draw seeded.

tests/_corner_scene.py at 200 x 152 fills no level past the fourth, has no equal Harris responses and no equal descriptors.  The builders
here reach what it does not: a frame that fills all 500 keypoints, equal responses, equal descriptors, a level with exactly n_l candidates,
a level whose interior is one pixel thick, no interior at all, a portrait frame, and hand-written score maps, descriptor sets and
displacement inputs for the entry points on their own.  What each builder reaches is asserted on the statement (tests/_orb_ref.py) in
tests/test_orb_stages_cpu.py; the figures below are the statement's on the CPU.

  full        _corner_scene's plane at twice the focal length, 416 x 312: [109 90 75 63 52 44 36 31] = 500 keypoints in both frames of the
              pair (the second frame translated by 2 PLANE_T, which moves the image as PLANE_T does at the original focal length), 332 matches
  blocks      random grey on a 5 x 5 block grid + integer noise in [-6, 6], three equal channels (every block junction is a corner)
                97 x 83    (seed 1)  32 and 7 keypoints at levels 0 and 1: far below every cut
                200 x 63   (seed 2)  the interior is the single row y = 31: 7 keypoints
                200 x 62             no interior at any level: 0 keypoints
                141 x 230  (seed 0)  portrait, levels 0-3 full
  periodic    blocks(64, 64, seed 0) tiled 3 x 4 = 256 x 192: 91 equal Harris responses, 91 duplicate descriptors, level 5 has exactly
              44 = n_5 candidates; paired with itself rolled by one period, so that equal descriptors meet across the frames
  mirror      blocks(150, 100, seed 7) beside its left-right flip, 200 x 150: 92 equal responses (the Sobel products are even under the
              flip), no equal descriptors
  checker     6-pixel squares of 0 and 255, 160 x 120: level 0 has no corner (a junction's pixels share one FAST score and the strict NMS
              drops them all) while level 1 is full; 92 equal responses, 72 duplicate descriptors
  noise       uniform random RGB, unequal channels, 160 x 120 (run as RGB and as BGR)
  constant    all 0 / all 255: the rounding of the grey and smoothing kernels at both ends of the byte

The seeds are the ones at which this file's generator meets the stated condition; another generator needs other seeds."""
import functools

import numpy as np

import _corner_scene as S
import _orb_ref as R
from bodyslam_amd import orb_tables as T

NF, NL = T.N_FEATURES, T.N_LEVELS
CHUNK = 4096                                        # pixels of one pass of the selector's compaction (256 threads x 16 bytes)


def level_view(st, name, frame, l):
    """level l of frame `frame` of the flat pyramid buffer st[name] as [H_l, W_l]"""
    w, h, off = st["levels"][l]
    return st[name][frame, off:off + w * h].reshape(h, w)


# ---- frames -------------------------------------------------------------------------------------------------------------------------------
def blocks(H, W, b=5, seed=0):
    rng = np.random.default_rng(seed)
    grid = rng.integers(0, 256, size=((H + b - 1) // b, (W + b - 1) // b))
    base = np.kron(grid, np.ones((b, b), dtype=np.int64))[:H, :W]
    g = np.clip(base + rng.integers(-6, 7, size=(H, W)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(g[..., None], 3, axis=2))


FULL_K, FULL_H, FULL_W = (400.0, 400.0, 208.0, 156.0), 312, 416


@functools.lru_cache(maxsize=None)
def full_pair():
    """((colour, depth), (colour, depth)) of the 416 x 312 pair"""
    a = S.render(S.translation_pose(np.zeros(3)), "plane", K=FULL_K, H=FULL_H, W=FULL_W)
    b = S.render(S.translation_pose(2.0 * S.PLANE_T), "plane", K=FULL_K, H=FULL_H, W=FULL_W)
    return a, b


def periodic():
    return np.tile(blocks(64, 64, seed=0), (3, 4, 1))


def mirror():
    m = blocks(150, 100, seed=7)
    return np.ascontiguousarray(np.concatenate([m, m[:, ::-1]], axis=1))


def checker():
    y, x = np.mgrid[0:120, 0:160]
    c = (((y // 6 + x // 6) % 2) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(c[..., None], 3, axis=2))


def noise():
    return np.random.default_rng(11).integers(0, 256, size=(120, 160, 3)).astype(np.uint8)


def constant(value, H=120, W=160):
    return np.full((H, W, 3), value, dtype=np.uint8)


# name -> (builder of the frames of one call [n, H, W, 3], bgr).  Two frames are a pair: the match runs on them.
FRAMES = {
    "full": (lambda: np.stack([full_pair()[0][0], full_pair()[1][0]]), False),
    "blocks_83x97": (lambda: np.stack([blocks(83, 97, seed=1), blocks(83, 97, seed=3)]), False),
    "blocks_63x200": (lambda: blocks(63, 200, seed=2)[None], False),
    "blocks_62x200": (lambda: blocks(62, 200, seed=0)[None], False),
    "blocks_230x141": (lambda: blocks(230, 141, seed=0)[None], False),
    "periodic": (lambda: np.stack([periodic(), np.roll(periodic(), 64, axis=1)]), False),
    "mirror": (lambda: mirror()[None], False),
    "checker": (lambda: checker()[None], False),
    "noise_rgb": (lambda: noise()[None], False),
    "noise_bgr": (lambda: noise()[None], True),
    "white": (lambda: constant(255)[None], False),
    "black": (lambda: constant(0)[None], False),
}


PAIRS = ("blocks_83x97", "full", "periodic")          # the entries of FRAMES with two frames


@functools.lru_cache(maxsize=None)
def frames(name):
    build, bgr = FRAMES[name]
    out = build()
    out.setflags(write=False)
    return out, bgr


@functools.lru_cache(maxsize=None)
def statement(name):
    """the statement of every frame of FRAMES[name] and, for a pair, of its match; computed once and shared"""
    rgb, bgr = frames(name)
    f = [R.extract(c[..., ::-1] if bgr else c) for c in rgb]
    m = R.match(f[0]["desc"], f[1]["desc"]) if len(f) == 2 else None
    return f, m


def equal_responses(f):
    """keypoints of one frame's statement whose Harris response equals that of another keypoint of the same level"""
    return sum(int(n - len(np.unique(f["resp"][f["kp"][:, 0] == l]))) for l, n in enumerate(f["counts"]))


def duplicate_descriptors(f):
    return len(f["desc"]) - len(np.unique(f["desc"], axis=0)) if len(f["desc"]) else 0


def candidates(f):
    return [int((s > 0).sum()) for s in f["score"]]


# ---- score maps for bs_orb_select -----------------------------------------------------------------------------------------------------------
SEL_H, SEL_W = 152, 200


@functools.lru_cache(maxsize=None)
def select_pyramid():
    return R.pyramid(R.grey(blocks(SEL_H, SEL_W, seed=0)))


def _interior(H, W):
    e = T.EDGE_THRESHOLD
    y, x = np.mgrid[e:H - e, e:W - e]
    return (y * W + x).reshape(-1)


def lattice_scores(groups):
    """level 0's score map uint8 [SEL_H, SEL_W] with, for every (k, score) of `groups`, k interior pixels at that score, each group
    spread evenly over the interior in row-major order; the groups do not overlap"""
    inner = _interior(SEL_H, SEL_W)
    score = np.zeros(SEL_H * SEL_W, dtype=np.uint8)
    free = np.ones(len(inner), dtype=bool)
    for k, s in groups:
        pool = np.flatnonzero(free)
        pick = pool[(np.arange(k, dtype=np.int64) * len(pool)) // k]
        score[inner[pick]] = s
        free[pick] = False
    return score.reshape(SEL_H, SEL_W)


# name -> the groups of lattice_scores; n_0 = 109, so the cut takes 218.  (The interior of a 200 x 152 level lies in the 4096-pixel chunks
# 1 to 5 of the 8: a score outside the interior is outside the contract.)
SELECT_CASES = {
    "ties_300": ((300, 50),),                       # T = 50, need = 218 of 300 ties over five chunks: the first 218 in pixel order win
    "exactly_2n": ((218, 50),),
    "exactly_n": ((109, 50),),
    "one": ((1, 50),),
    "need_1": ((217, 60), (50, 50)),                # T = 50, need = 1: the first of the 50 ties only
}


def select_case(name):
    """(grey levels, score maps per level, hist int32 [8, 256] as bs_orb_fast leaves it: np.bincount of each map, bin 0 not counted)"""
    g = select_pyramid()
    score = [lattice_scores(SELECT_CASES[name])] + [np.zeros_like(a) for a in g[1:]]
    hist = np.stack([np.bincount(s.reshape(-1), minlength=256) for s in score]).astype(np.int32)
    hist[:, 0] = 0
    return g, score, hist


def cut_of(score, n):
    """(T, need, ties) of the selector's cut on one score map: the largest T with #(score >= T) >= 2 n, how many of the pixels at T it
    takes, how many there are; (0, 0, 0) when the map has fewer than 2 n candidates"""
    h = np.bincount(score.reshape(-1), minlength=256)
    acc = 0
    for s in range(255, 0, -1):
        if acc + h[s] >= 2 * n:
            return s, 2 * n - acc, int(h[s])
        acc += h[s]
    return 0, 0, 0


# ---- descriptor sets for bs_orb_match / bs_orb_match_pairs ----------------------------------------------------------------------------------
def _random_desc(rng, *shape):
    return rng.integers(0, 1 << 32, size=shape + (8,), dtype=np.uint64).astype(np.uint32)


def _flip_bits(rng, d, k):
    """d uint32 [n, 8] with k distinct random bits of every row flipped"""
    out = d.copy()
    for i in range(len(d)):
        for b in rng.choice(256, size=k, replace=False):
            out[i, b // 32] ^= np.uint32(1) << np.uint32(b % 32)
    return out


def match_case(name):
    """(desc uint32 [frames, 500, 8], counts int32 [frames]): rows at and behind a frame's count hold random bits, which the match must
    not read into its result.  A count outside 0 .. 500 is clamped by the kernel; clamped() gives what it then works on."""
    rng = np.random.default_rng(sum(name.encode()))
    if name.startswith("random_"):
        n1, n2 = (int(v) for v in name.split("_")[1:])
        return _random_desc(rng, 2, NF), np.array([n1, n2], dtype=np.int32)
    if name == "identical_64":                      # every distance is 0: every query's best train is 0, every train's best query is 0
        d = _random_desc(rng, 2, NF)
        d[:, :64] = d[0, 0]
        return d, np.array([64, 64], dtype=np.int32)
    if name == "triples":                           # 160 descriptors, each three times, shuffled differently in the two frames (3 x 200 would pass 500)
        base = _random_desc(rng, 160)
        d = _random_desc(rng, 2, NF)
        for f in (0, 1):
            d[f, :480] = np.repeat(base, 3, axis=0)[rng.permutation(480)]
        return d, np.array([480, 480], dtype=np.int32)
    if name == "one_distance":                      # train perm[i] = query i with 3 bits flipped: 400 matches, all at distance 3
        d = _random_desc(rng, 2, NF)
        d[1, rng.permutation(400)] = _flip_bits(rng, d[0, :400], 3)
        return d, np.array([400, 400], dtype=np.int32)
    if name == "clamped_counts":                    # 10^6 -> 500, -5 -> 0; three frames = two consecutive pairs
        return _random_desc(rng, 3, NF), np.array([10 ** 6, 300, -5], dtype=np.int32)
    raise KeyError(name)


MATCH_CASES = ("random_500_500", "random_500_1", "random_1_500", "random_0_300", "random_300_0", "random_257_256", "identical_64", "triples",
               "one_distance", "clamped_counts")


def clamped(desc, counts):
    return [desc[f, :min(max(int(c), 0), NF)] for f, c in enumerate(counts)]


def shared_best(dq, dt):
    """queries whose best Hamming distance is reached by two or more trains"""
    if len(dq) == 0 or len(dt) == 0:
        return 0
    bq = np.unpackbits(dq.view(np.uint8).reshape(len(dq), 32), axis=1).astype(np.int16)
    bt = np.unpackbits(dt.view(np.uint8).reshape(len(dt), 32), axis=1).astype(np.int16)
    D = (bq[:, None, :] != bt[None, :, :]).sum(-1)
    return int(((D == D.min(1, keepdims=True)).sum(1) >= 2).sum())


# ---- inputs for bs_orb_displacement ---------------------------------------------------------------------------------------------------------
DISP_CASES = ("zeros", "nan", "no_match", "all_zero", "fewer_curr")


def displacement_case(name):
    """dict(pt fp32 [2, 500, 2], counts [2], matches int32 [500, 3], M, depth fp32 [2, FULL_H, FULL_W], K): 500 (fewer_curr: 300) matches
    between the points of two frames, every point at a pixel of its own.  Depth in (0.2, 1] m, |u - cx| / fx <= 0.52.
      zeros       depth 0 under every third point, at different points in the two frames (the reference mode's zip misaligns); point 1 of
                  both frames at x = W - 0.5 (read at W - 1), point 2 at x = W exactly (outside), point 4 at x = -0.5 (read at 0)
      nan         the same with NaN under two points of each frame: NaN is not 0, the pair counts and the mean is NaN
      no_match    M = 0;  all_zero  every depth 0: both give NaN and no pair
      fewer_curr  n2 = 300 < n1 = 500: the reference mode's swapped lookup skips q >= n2"""
    rng = np.random.default_rng(5)
    H, W = FULL_H, FULL_W
    n = [NF, 300 if name == "fewer_curr" else NF]
    pt = np.zeros((2, NF, 2), dtype=np.float32)
    for f in (0, 1):
        pix = rng.choice(H * (W - 2), size=NF, replace=False)           # (columns 1 .. W - 2: the edge columns belong to the points below)
        pt[f, :, 0] = (pix % (W - 2) + 1) + rng.integers(0, 4, size=NF) * 0.25
        pt[f, :, 1] = (pix // (W - 2)) + rng.integers(0, 4, size=NF) * 0.25
        pt[f, 1, 0], pt[f, 2, 0], pt[f, 4, 0] = W - 0.5, float(W), -0.5
    M = 0 if name == "no_match" else min(n)
    matches = np.stack([rng.permutation(n[0])[:min(n)], rng.permutation(n[1])[:min(n)], np.sort(rng.integers(0, 90, size=min(n)))], 1).astype(np.int32)
    depth = (0.2 + 0.8 * rng.random(size=(2, H, W))).astype(np.float32)
    inside = lambda f, k: 0 <= int(pt[f, k, 0]) < W
    if name == "all_zero":
        depth[:] = 0.0
    else:
        for f, r in ((0, 0), (1, 1)):
            for k in list(range(r, NF, 3)) + (list(range(2, 60, 3)) if f else []):          # (20 more in the current frame: nA != nB)
                if inside(f, k):
                    depth[f, int(pt[f, k, 1]), int(pt[f, k, 0])] = 0.0
    if name == "nan":
        for f, ks in ((0, (5, 200)), (1, (80, 101))):
            for k in ks:
                depth[f, int(pt[f, k, 1]), int(pt[f, k, 0])] = np.nan
    return dict(pt=pt, counts=np.array(n, dtype=np.int32), matches=matches, M=M, depth=depth, K=FULL_K)


def displacement_statement(c, association):
    n = c["counts"]
    return R.displacement(c["pt"][0, :n[0]], c["pt"][1, :n[1]], c["matches"][:c["M"]].astype(np.int64), c["depth"][0], c["depth"][1], c["K"], association)


# ---- the batch of five ----------------------------------------------------------------------------------------------------------------------
def batch_of_five(H=120, W=160):
    """blocks, a constant frame, periodic cropped, blocks with another seed, a constant frame: pairs (0, 1), (1, 2) and (3, 4) touch a frame
    without keypoints"""
    return np.stack([blocks(H, W, seed=4), constant(90, H, W), np.ascontiguousarray(periodic()[:H, :W]), blocks(H, W, seed=6), constant(255, H, W)])
