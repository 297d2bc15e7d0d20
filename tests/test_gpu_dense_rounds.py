"""dense_rounds (garden_amd/csrc/gv_dense_rounds.hpp) is how cull_hot_kernel<true, K> settles a super-tile's corner candidates: listed
in LDS, decided 256 at a time, the ballot words rebuilt from ORed bits. A test-only kernel (tests/dense_rounds_probe.hip) compiles the
same header with a table as the decision, one super-tile of K tiles per workgroup, and its ballot words, per-chunk totals and isVisible
bytes are compared with numpy: K = 2 and 4, one super-tile and three with the third ending one entry into its last tile, no candidate,
all candidates, exactly one round and one entry more, a lone candidate in the last lane, one wave only, all invisible, random fills.
The decision itself counts an error when it is asked about an entry that is no candidate or is handed the wrong class."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TILE, TILES_PER_CHUNK = 256, 4
OUTSIDE, INSIDE, UNDECIDED = 0, 1, 2
WORD_GUARD, BYTE_GUARD = 0xA5A5A5A5A5A5A5A5, 7


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """tests/dense_rounds_probe.hip built for gfx950 with the library's own flags"""
    out = str(tmp_path_factory.mktemp("dense_rounds_probe") / "libdense_rounds_probe.so")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                    "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize", "-shared", "-I",
                    os.path.join(HERE, "..", "garden_amd", "csrc"), os.path.join(HERE, "dense_rounds_probe.hip"), "-o", out], check=True)
    import torch  # noqa: F401  (one HIP runtime per process: torch's first, as garden_amd.lib does)
    lib = C.CDLL(out)
    P, u32 = C.c_void_p, C.c_uint32
    lib.dense_rounds_probe.argtypes = [u32, P, P, P, P, P, P, u32, u32]
    lib.dense_rounds_probe.restype = C.c_int
    return lib


def sizes(k):
    """one super-tile; three, the third ending one entry into its last tile"""
    return {"one": k * TILE, "three": 2 * k * TILE + (k - 1) * TILE + 1}


def classes(rng, n, chosen):
    cls = np.zeros(n, dtype=np.uint8)
    cls[chosen] = rng.choice([INSIDE, UNDECIDED], size=len(chosen)).astype(np.uint8)
    return cls


def pattern(name, n, k, rng):
    """(cls, vis) per entry; vis of an entry that is no candidate is noise the kernel must not read into its outputs"""
    span = k * TILE                      # a super-tile
    full = (n // span - 1) * span        # the first entry of the last full super-tile
    vis = rng.integers(0, 2, n).astype(np.uint8)
    if name == "none":
        return np.zeros(n, dtype=np.uint8), vis
    if name == "all_visible":
        return classes(rng, n, np.arange(n)), np.ones(n, dtype=np.uint8)
    if name in ("exactly_256", "exactly_257"):
        chosen = full + rng.choice(span, 256 if name == "exactly_256" else 257, replace=False)
        return classes(rng, n, np.sort(chosen)), vis
    if name == "last_lane":  # lane 63 of the last wave of the last tile of every full super-tile, and the array's last entry
        chosen = np.unique(np.append(np.arange(span - 1, n, span), n - 1))
        cls = classes(rng, n, chosen)
        vis[chosen] = 1
        return cls, vis
    if name == "one_wave":
        return classes(rng, n, np.flatnonzero((np.arange(n) % TILE) // 64 == 2)), vis
    if name == "all_invisible":
        cls = classes(rng, n, np.flatnonzero(rng.random(n) < 0.39))
        vis[cls != OUTSIDE] = 0
        return cls, vis
    share = {"random_1": 0.01, "random_39": 0.39, "random_90": 0.90}[name]
    return classes(rng, n, np.flatnonzero(rng.random(n) < share)), vis


PATTERNS = ["none", "all_visible", "exactly_256", "exactly_257", "last_lane", "one_wave", "all_invisible", "random_1", "random_39", "random_90"]


def run(probe, k, cls, vis, write_bytes=True):
    import torch
    n = len(cls)
    nblocks = (n + TILE - 1) // TILE
    launched = (nblocks + k - 1) // k * k  # tiles the grid covers: the ones past nblocks must not be stored
    dev = torch.device("cuda:0")
    d_cls, d_vis = torch.from_numpy(cls).to(dev), torch.from_numpy(vis).to(dev)
    d_mask = torch.from_numpy(np.full(launched * 4 + 8, WORD_GUARD, dtype=np.uint64).view(np.int64)).to(dev)
    d_chunks = torch.zeros((nblocks + TILES_PER_CHUNK - 1) // TILES_PER_CHUNK + 1, dtype=torch.int32, device=dev)
    d_bytes = torch.full((launched * TILE + TILE,), BYTE_GUARD, dtype=torch.uint8, device=dev)
    d_err = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rc = probe.dense_rounds_probe(k, d_cls.data_ptr(), d_vis.data_ptr(), d_mask.data_ptr(), d_chunks.data_ptr(),
                                  d_bytes.data_ptr() if write_bytes else None, d_err.data_ptr(), n, TILES_PER_CHUNK)
    assert rc == 0
    return (d_mask.cpu().numpy().view(np.uint64), d_chunks.cpu().numpy().astype(np.int64), d_bytes.cpu().numpy(), int(d_err.cpu()[0]), nblocks)


def expected(cls, vis):
    n = len(cls)
    nblocks = (n + TILE - 1) // TILE
    visible = np.zeros(nblocks * TILE, dtype=np.uint8)
    visible[:n] = (cls != OUTSIDE) & (vis != 0)
    words = np.packbits(visible.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).ravel()
    per_tile = visible.reshape(nblocks, TILE).sum(axis=1)
    chunks = np.add.reduceat(per_tile, np.arange(0, nblocks, TILES_PER_CHUNK))
    return words, chunks, visible[:n]


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("extent", ["one", "three"])
@pytest.mark.parametrize("k", [2, 4])
def test_dense_rounds_outputs_equal_numpy(probe, k, extent, name):
    n = sizes(k)[extent]
    rng = np.random.Generator(np.random.PCG64(1000 * k + n + PATTERNS.index(name)))
    cls, vis = pattern(name, n, k, rng)
    if name in ("exactly_256", "exactly_257"):
        assert int((cls != OUTSIDE).sum()) == int(name[-3:])
    if name not in ("none", "last_lane"):
        assert set(np.unique(cls[cls != OUTSIDE])) == {INSIDE, UNDECIDED}  # both classes among the candidates
    words, chunks, visible = expected(cls, vis)
    got_words, got_chunks, got_bytes, errors, nblocks = run(probe, k, cls, vis)
    assert errors == 0
    assert np.array_equal(got_words[:nblocks * 4], words)
    assert np.all(got_words[nblocks * 4:] == np.uint64(WORD_GUARD))  # tiles past the array's last: not stored
    assert np.array_equal(got_chunks[:-1], chunks) and got_chunks[-1] == 0
    assert np.array_equal(got_bytes[:n], visible)
    assert np.all(got_bytes[n:] == BYTE_GUARD)


@pytest.mark.parametrize("k", [2, 4])
def test_without_is_visible_bytes(probe, k):
    """an emitting view: the bytes are the emit kernel's, the cull stores none"""
    n = sizes(k)["three"]
    rng = np.random.Generator(np.random.PCG64(77 + k))
    cls, vis = pattern("random_39", n, k, rng)
    cls[2 * k * TILE:] = OUTSIDE  # ... and the last super-tile takes the exit of one without a candidate
    words, chunks, _ = expected(cls, vis)
    got_words, got_chunks, got_bytes, errors, nblocks = run(probe, k, cls, vis, write_bytes=False)
    assert errors == 0
    assert np.array_equal(got_words[:nblocks * 4], words)
    assert np.array_equal(got_chunks[:-1], chunks)
    assert np.all(got_bytes == BYTE_GUARD)
