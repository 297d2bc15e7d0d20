"""Test helpers of the Hi-Z pyramid's build paths: which kernel hiz_reduce (garden_amd/csrc/gv_context.cpp) launches for which
levels of an image of a given size, restated in plain Python (hiz_plan), the image sizes that between them take every path
(SIZES), and the depth image of test_hiz_pyramid_parity (special_depth). TEST INFRASTRUCTURE ONLY.

The plan depends on the level sizes alone, never on the texels, the reduction rule or the texel format: a size is in the
same class under both rules."""
import ctypes as C
import functools
import os
import re

import numpy as np

from garden_amd import scene

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "garden_amd", "csrc")


def source_text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def header_constant(header, name):
    """the value of `constexpr uint32_t <name> = <digits>;` in a header of the library, read as text"""
    m = re.search(r"constexpr\s+uint32_t\s+" + re.escape(name) + r"\s*=\s*(\d+)\s*;", source_text(header))
    assert m, f"{name} not found in {header}"
    return int(m.group(1))


TAIL_TEXELS = header_constant("gv_kernels.hpp", "kHizTailTexels")
# Literals of the dispatch, each with the line of the library that holds it (test_hiz_plan_census.py checks that it still does).
FOUR_MIN_GROUPS = 96     # gv_context.cpp hiz_reduce: "((ctx->mip_w[k] + 63) / 64) * ((ctx->mip_h[k] + 63) / 64) >= 96"
FOUR_MAX_GROUPS = 200    # gv_context.cpp hiz_reduce: "((ctx->mip_w[k] + 63) / 64) * ((ctx->mip_h[k] + 63) / 64) <= 200"
MAX_SIDE = 32768         # gv_context.cpp gv_hiz_build: "width > 32768 || height > 32768" is refused
TWO_TILE_MIN_PAIRS = 1024  # gv_hiz.hip launch_hiz_fused: "(sw / 128) * (sh / 64) >= 1024"
LITERAL_LINES = {
    "gv_context.cpp": ["((ctx->mip_w[k] + 63) / 64) * ((ctx->mip_h[k] + 63) / 64) >= %d &&" % FOUR_MIN_GROUPS,
                       "((ctx->mip_w[k] + 63) / 64) * ((ctx->mip_h[k] + 63) / 64) <= %d &&" % FOUR_MAX_GROUPS,
                       "sw % 64 == 0 && sh % 64 == 0 && k + 5 < ctx->hiz_mips",
                       "(uint64_t)ctx->mip_w[k] * ctx->mip_h[k] <= kHizTailTexels",
                       "(uint64_t)ctx->mip_w[k + 2] * ctx->mip_h[k + 2] > kHizTailTexels && (uint64_t)ctx->mip_w[k + 3] * ctx->mip_h[k + 3] > kHizTailTexels / 2",
                       "k + 3 < ctx->hiz_mips && sw >= 2 && sh >= 2 &&",
                       "k + 2 < ctx->hiz_mips && sw >= 2 && sh >= 2",
                       "width > %d || height > %d" % (MAX_SIDE, MAX_SIDE)],
    "gv_hiz.hip": ["src_depth && sw % 128 == 0 && (sw / 128) * (sh / 64) >= " + str(TWO_TILE_MIN_PAIRS)],
}

BRANCHES = ("six_one_tile", "six_two_tiles", "tail", "four", "three", "single")
SOURCES = ("depth", "pairs")
LEVELS = {"six_one_tile": 6, "six_two_tiles": 6, "four": 4, "three": 3, "single": 1}  # (the tail takes all that are left)


def mip_sizes(w, h, rule=0):
    """[(w, h)] of every level, 0 first, as oracle.Hiz(depth, rule).level(k).shape gives them: read from the layout the oracle
    computes for an image of this size (gvo_hiz_layout, what Hiz.__init__ calls), without building a pyramid. (The rule decides
    texel values only.)"""
    from oracle import oracle_py
    c = oracle_py.GvoHiz()
    oracle_py.load().gvo_hiz_layout(w, h, C.byref(c))
    return [(int(c.mip_w[k]), int(c.mip_h[k])) for k in range(c.mip_count)]


def groups64(size):
    return ((size[0] + 63) // 64) * ((size[1] + 63) // 64)


def texels(size):
    return size[0] * size[1]


def hiz_plan(sizes):
    """The launches of hiz_reduce + launch_hiz_fused for a pyramid with these level sizes: [(branch, k, source)], k = the first
    level the launch writes, source = "depth" when it reads the depth image (k == 1), else "pairs"."""
    mips = len(sizes)
    plan = []
    k = 1
    while k < mips:
        sw, sh = sizes[k - 1]
        source = "depth" if k == 1 else "pairs"
        if sw % 64 == 0 and sh % 64 == 0 and k + 5 < mips:
            two = source == "depth" and sw % 128 == 0 and (sw // 128) * (sh // 64) >= TWO_TILE_MIN_PAIRS
            plan.append(("six_two_tiles" if two else "six_one_tile", k, source))
            k += 6
        elif texels(sizes[k]) <= TAIL_TEXELS:
            plan.append(("tail", k, source))
            k = mips
        elif (k + 3 < mips and sw >= 2 and sh >= 2 and FOUR_MIN_GROUPS <= groups64(sizes[k]) <= FOUR_MAX_GROUPS and
              texels(sizes[k + 2]) > TAIL_TEXELS and texels(sizes[k + 3]) > TAIL_TEXELS // 2):
            plan.append(("four", k, source))
            k += 4
        elif k + 2 < mips and sw >= 2 and sh >= 2:
            plan.append(("three", k, source))
            k += 3
        else:
            plan.append(("single", k, source))
            k += 1
    return plan


def four_but_for_groups(sizes, k):
    """every condition of the four-level form holds for a launch at level k except, perhaps, the workgroup count"""
    sw, sh = sizes[k - 1]
    return (k + 3 < len(sizes) and sw >= 2 and sh >= 2 and texels(sizes[k + 2]) > TAIL_TEXELS and
            texels(sizes[k + 3]) > TAIL_TEXELS // 2 and texels(sizes[k]) > TAIL_TEXELS and
            not (sw % 64 == 0 and sh % 64 == 0 and k + 5 < len(sizes)))


def level1_virtual(sizes):
    """gv_hiz_build: level 1 is not stored when the first six levels come from the six-level kernel"""
    return sizes[0][0] % 64 == 0 and sizes[0][1] % 64 == 0 and len(sizes) > 6


def reads_rule(sizes):
    """some level that is reduced has an odd size (above one texel: a footprint clamped onto a single row or column holds the same
    texels under both rules): only then can a texel depend on the rule"""
    return any((sw > 1 and sw % 2 == 1) or (sh > 1 and sh % 2 == 1) for sw, sh in sizes[:-1])


def base_depth(w, h, seed=scene.SEED):
    """walls only (scene.synthetic_depth): the image of the occlusion queries"""
    return scene.synthetic_depth(w, h, seed=seed)


@functools.lru_cache(maxsize=2)
def special_depth(w, h, seed=None):
    """The depth image of test_hiz_pyramid_parity (tests/test_gpu_cull.py): synthetic_depth with 37 walls, noise below 0.01, and
    the ten values the comparisons treat specially — +0 / -0, NaN, the infinities, half subnormals, underflow, overflow — at
    max(1, w * h // 23) texels each. The reduction order of hiz.frag:29-60 is part of the contract; these pin it.
    Read-only (shared between the tests that build from it)."""
    depth = scene.synthetic_depth(w, h, rects=37)
    rng = np.random.default_rng(w * 131 + h if seed is None else seed)
    depth = np.maximum(depth, (rng.random((h, w)) * 0.01).astype(np.float32))
    k = max(1, (w * h) // 23)
    flat = depth.reshape(-1)
    for value in (0.0, -0.0, np.nan, np.inf, -np.inf, 3e-6, -3e-6, 1e-9, 7e4, -7e4):
        flat[rng.choice(flat.size, k, replace=False)] = np.float32(value)
    depth.setflags(write=False)
    return depth


# gv_hiz_build refuses these (a side beyond MAX_SIDE); (40000, 1) would be the smallest image whose single-level launch reads pairs
REFUSED = [(40000, 1), (1, 40000), (MAX_SIDE + 1, 1), (1, MAX_SIDE + 1)]
# One or two levels: nothing, or one tail launch of one texel.
DEGENERATE = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 1), (1, 3)]
SIZES = DEGENERATE + [
    # the single-level kernel: a one-texel-high / -wide source whose next level is still beyond the tail; from depth, then tail
    (20000, 1), (1, 20000),
    # ... at the longest side gv_hiz_build takes: the tail's first level then has exactly kHizTailTexels texels. (The single-level
    # kernel would read pairs only behind a first level of more than 2 * kHizTailTexels texels in a line: a side beyond MAX_SIDE.)
    (32768, 1), (1, 32768),
    # the tail from the depth image with exactly kHizTailTexels texels in its first level (128 x 64), odd source
    (257, 129),
    # six-level kernel, level 6 odd (3 x 5, 5 x 3) or one texel wide / high, then the tail from those pairs; width 64 and 192: not 128 | w
    (192, 320), (320, 192), (64, 128), (64, 4096), (4096, 64),
    # two tiles per workgroup at exactly 1024 pairs, tall and wide
    (2048, 4096), (8192, 1024),
    # 128 | w, 1008 pairs: one tile per workgroup on a grid of 2016
    (2048, 4032),
    # six-level kernel from pairs on a 1 x 2 grid (the texel cap of the census admits this one)
    (4096, 8192),
    # ... and behind a three-level launch, on 1 x 1 and 1 x 2: the level it reads starts 259 * 259 + 129 * 129 texels into the
    # pyramid (even: 16-byte aligned as float2, 8 mod 16 bytes as packed halfs) resp. 259 * 514 + 129 * 257 (odd: 8 resp. 4 mod 16)
    (518, 518), (518, 1028),
    # the four-level kernel at 96 and at 200 workgroups; 95 and 201: three levels
    (1537, 1023), (2561, 1281), (2433, 641), (8501, 301),
    # ... with an odd source width, height, both
    (1921, 1081), (1601, 899), (1919, 1079),
    # ... as thin as it gets (172 x 1 workgroups; level 4 is 3 x 1375, any thinner leaves it under 4096 texels), then the tail from that
    (51, 22001), (22001, 51),
]

# The sizes of test_hiz_pyramid_parity (tests/test_gpu_cull.py), which the census counts as covered.
PARITY_SIZES = [(64, 64), (5, 3), (7, 7), (135, 77), (1920, 1080), (4096, 4096), (1024, 512), (257, 131), (515, 389), (1283, 719),
                (1000, 37), (2560, 1440), (3840, 2160), (2049, 1025), (20000, 3), (3, 20000), (16400, 2), (1600, 900)]


# Builds on ONE context, in this order (size, seed of the image): large -> tiny -> a frame size -> one tile -> one texel high ->
# odd level 6 -> the first size again with another image. Level 1 is virtual for the sizes divisible by 64 and stored for the others
# (hiz_level1_virtual / hiz_level1_stored flip at every step but one), the level offsets change every time, the allocation is
# made by the first build and reused by the rest.
SEQUENCE = [((4096, 4096), 1), ((5, 3), 2), ((1920, 1080), 3), ((64, 64), 4), ((20000, 1), 5), ((192, 320), 6), ((4096, 4096), 7)]


def plan_of(size):
    return hiz_plan(mip_sizes(*size))


def branch_pairs(sizes_list):
    """{(branch, source): the smallest size of the list (in texels) whose plan holds it}"""
    out = {}
    for size in sorted(sizes_list, key=lambda s: (texels(s), s)):
        for branch, _k, source in plan_of(size):
            out.setdefault((branch, source), size)
    return out


# The sizes whose pyramids the occlusion queries run against: the smallest of SIZES for every (branch, source), and every
# degenerate size. (Among them sizes one texel high or wide.)
QUERY_SIZES = sorted(set(DEGENERATE) | set(branch_pairs(SIZES).values()), key=lambda s: (texels(s), s))


def cull_both(vis, oracle, sc, view, hz):
    """One Hi-Z cull of the bound scene on the GPU and by the oracle against its pyramid `hz`; returns (got, exp, exp_vis)."""
    vis.cull(0, [view])
    got = vis.fetch(0, write_back=False, occupancy=sc.count)
    meshes = sc.meshes.copy()
    meshes["isVisible"] = 7  # the main pass overwrites every slot
    exp = oracle.prepare_meshes(meshes, sc.transforms, sc.entity_to_transform, view, hiz=hz)
    return got, exp, meshes["isVisible"]


def assert_cull_equal(got, exp, exp_vis, what=""):
    assert got["draw_count"] == exp["draw_count"], what
    assert np.array_equal(got["visible_idx"], exp["visible_idx"]), what
    assert np.array_equal(got["distance_sq"].view(np.uint32), exp["distance_sq"].view(np.uint32)), what
    assert got["is_visible"] is not None and np.array_equal(got["is_visible"], exp_vis), what


def assert_pyramid_equal(vis, exp, what=""):
    """every level >= 1 of the context's pyramid equals the oracle's `exp` bit for bit"""
    assert vis.hiz_mip_count() == exp.mip_count, what
    for k in range(1, exp.mip_count):
        e = exp.level(k)
        g = vis.hiz_read_level(k, e.shape[1], e.shape[0])
        if not np.array_equal(g.view(np.uint32), e.view(np.uint32)):
            bad = np.argwhere(g.view(np.uint32) != e.view(np.uint32))
            raise AssertionError(f"{what} mip {k} ({e.shape[1]} x {e.shape[0]}) differs at {len(bad)} components, first (y, x, c) = {bad[0].tolist()}: "
                                 f"got {g[tuple(bad[0])]!r}, expected {e[tuple(bad[0])]!r}")
