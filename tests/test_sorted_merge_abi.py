"""gv_merge_sorted on the CPU tier: the header declares the three entry points and both structs and the library exports them,
GvMergeItem / GvMergeGroup have the C layout in ctypes under C99 and C++11, and the C twin of the merge order (tests/merge_twin.h)
equals a numpy stable sort of the concatenated lists."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import merge_support as msup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gv_merge_sorted", "gv_merge_device", "gv_merge_fetch")


def test_header_declares_and_library_exports_the_entry_points():
    from garden_amd import lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "garden_vis.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in lib.EXPORTS, name
    for struct in ("GvMergeItem", "GvMergeGroup"):
        assert re.search(r"typedef\s+struct\s+%s\s*\{[^}]*\}\s*%s\s*;" % (struct, struct), text), struct
    assert re.search(r"#define GV_MAX_MERGE_GROUPS 12u\b", text) and re.search(r"#define GV_MAX_MERGE_ITEMS 16u\b", text)
    assert lib.GV_MAX_MERGE_GROUPS == 12 and lib.GV_MAX_MERGE_ITEMS == 16
    if os.path.exists(lib.LIB_PATH):
        handle = lib.load()
        for name in SYMBOLS:
            assert hasattr(handle, name), name
        assert handle.gv_abi_version() == 4
    assert re.search(r"#define GV_ABI_VERSION 4u?\b", text)


@pytest.mark.parametrize("compiler", [["gcc", "-std=c99", "-pedantic"], ["g++", "-std=c++11", "-pedantic", "-x", "c++"]], ids=["c99", "cxx11"])
def test_merge_structs_match_the_header(tmp_path, compiler):
    from garden_amd import lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "garden_vis.h"', "int main(void) {"]
    for cls in (lib.GvMergeItem, lib.GvMergeGroup):
        lines.append(f'    printf("%zu", sizeof({cls.__name__}));')
        for field, _ in cls._fields_:
            lines.append(f'    printf(" %zu", offsetof({cls.__name__}, {field}));')
        lines.append('    printf("\\n");')
    lines += ["    return 0;", "}"]
    src = tmp_path / "merge_abi.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "merge_abi"
    subprocess.run(compiler + ["-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    rows = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    for cls, row, size, at in ((lib.GvMergeItem, rows[0], 16, [0, 4, 8, 12]),
                               (lib.GvMergeGroup, rows[1], 56, [0, 4, 8, 16, 20, 24, 28, 32, 36, 40, 48])):
        got_size, *offsets = [int(x) for x in row.split()]
        assert got_size == ctypes.sizeof(cls) == size
        assert offsets == [getattr(cls, f).offset for f, _ in cls._fields_] == at


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return msup.build_twin(tmp_path_factory.mktemp("merge_twin"))


def sorted_list(keys, descending):
    """float32 keys in the sort's own order"""
    bits = np.asarray(keys, np.float32).view(np.uint32)
    order = np.argsort(msup.key_of(bits), kind="stable")
    return bits[order[::-1] if descending else order].view(np.float32)


def same_order(twin, lists, descending):
    got = msup.twin_order(twin, lists, descending)
    exp = msup.numpy_order(lists, descending)
    assert got[0].tolist() == exp[0].tolist() and got[1].tolist() == exp[1].tolist()
    return got


def test_twin_key_is_the_sorts_key_order(twin):
    values = np.array([-np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-40, 2.0, np.inf], np.float32)
    keys = [twin.twin_key(int(b)) for b in values.view(np.uint32)]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)  # -0.0 sorts below +0.0
    assert keys == msup.key_of(values.view(np.uint32)).tolist()


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("lists", [1, 2, 3, 8, 16])
def test_twin_random_keys(twin, lists, descending):
    rng = np.random.Generator(np.random.PCG64(lists))
    sizes = rng.choice([0, 1, 63, 64, 65, 257, 1025, 4097], lists)
    # a small alphabet as well: many ties inside and across the lists
    for draw in (lambda n: rng.uniform(0, 1e6, n), lambda n: rng.integers(0, 8, n).astype(np.float32)):
        same_order(twin, [sorted_list(draw(int(n)), descending) for n in sizes], descending)


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
def test_twin_identical_lists_tie_in_list_order(twin, descending):
    one = sorted_list(np.random.Generator(np.random.PCG64(5)).integers(0, 50, 300).astype(np.float32), descending)
    which, index = same_order(twin, [one.copy() for _ in range(16)], descending)
    # every key is tied across every list: each run of equal keys is walked list by list, each list's records in their own order
    merged = np.stack([which, index], axis=1)
    keys = one[index]
    for k in np.unique(keys):
        run = merged[keys == k]
        assert run[:, 0].tolist() == sorted(run[:, 0].tolist())
        for l in range(16):
            mine = run[run[:, 0] == l][:, 1]
            assert mine.tolist() == sorted(mine.tolist())


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
def test_twin_negative_zero_and_infinite_keys(twin, descending):
    rng = np.random.Generator(np.random.PCG64(9))
    special = np.array([-np.inf, -7.25, -1.0, -0.0, 0.0, 1.0, 7.25, np.inf], np.float32)
    lists = [sorted_list(np.concatenate([rng.choice(special, 40), rng.normal(0, 5, 100).astype(np.float32)]), descending) for _ in range(5)]
    which, index = same_order(twin, lists, descending)
    merged = np.array([lists[l][i] for l, i in zip(which, index)], np.float32)
    t = msup.key_of(merged.view(np.uint32)).astype(np.int64)
    assert (np.diff(t) <= 0).all() if descending else (np.diff(t) >= 0).all()
    zeros = merged.view(np.uint32)[merged == 0]
    assert len(set(zeros.tolist())) == 2  # both zeros are there, and T keeps all of one kind in front of the other
    assert (np.diff(msup.key_of(zeros).astype(np.int64)) <= 0).all() if descending else (np.diff(msup.key_of(zeros).astype(np.int64)) >= 0).all()
