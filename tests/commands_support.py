"""Test helpers of gv_pool_emit_draw_commands: the expected command bytes as a numpy restatement of the rule (DESIGN.md §4 item 10,
include/garden_vis.h), written from the rule and not from the kernels, and the command layouts the tests use as numpy structured
dtypes. TEST INFRASTRUCTURE ONLY."""
import numpy as np

BACKGROUND = 0xA5


def layout_dtype(stride, count, instance_count, first, first_instance, vertex_offset=None, draw=None):
    """The command struct as a numpy structured dtype (fields at explicit offsets)."""
    names = ["count", "instance_count", "first", "first_instance"]
    formats = [np.uint32] * 4
    offsets = [count, instance_count, first, first_instance]
    if vertex_offset is not None:
        names.append("vertex_offset"), formats.append(np.int32), offsets.append(vertex_offset)
    if draw is not None:
        names.append("draw"), formats.append(np.uint32), offsets.append(draw)
    return np.dtype(dict(names=names, formats=formats, offsets=offsets, itemsize=stride))


# indexed, 20 bytes: indexCount, instanceCount, firstIndex, vertexOffset, firstInstance
INDEXED = layout_dtype(20, count=0, instance_count=4, first=8, first_instance=16, vertex_offset=12)
# non-indexed, 16 bytes: vertexCount, instanceCount, firstVertex, firstInstance
PLAIN = layout_dtype(16, count=0, instance_count=4, first=8, first_instance=12)
# 32 bytes with the draw's number, fields out of order, gaps at 0 .. 4 and 24 .. 28
GAPS = layout_dtype(32, count=8, instance_count=4, first=20, first_instance=28, vertex_offset=16, draw=12)
# the indexed command at the front of a 64-byte struct, the draw's number in its last word
WIDE = layout_dtype(64, count=0, instance_count=4, first=8, first_instance=16, vertex_offset=12, draw=60)


def background(rows, stride):
    return np.full((rows, stride), BACKGROUND, np.uint8)


def geometry_table(rows):
    """rows of (count, first, vertex_offset) as the structured array GpuVisibility.bind_geometry takes"""
    table = np.zeros(len(rows), np.dtype([("count", np.uint32), ("first", np.uint32), ("vertex_offset", np.int32)]))
    for k, (count, first, vertex_offset) in enumerate(rows):
        table[k] = (count, first, vertex_offset)
    return table


def view_commands(slots, first, ids, table, merge):
    """The commands of ONE view as a list of dicts, from the rule: `slots` = visible_idx[0 .. n) in delivery order (POOL slots),
    first[0 .. n] = first_k with the closing word starts[v + 1] behind the last draw, `ids` per pool slot (None: every id is 0)."""
    n = len(slots)
    g = [0 if ids is None else int(ids[int(s)]) for s in slots]
    if merge:
        heads = [k for k in range(n) if k == 0 or g[k] != g[k - 1]]
    else:
        heads = list(range(n))
    out = []
    for r, h in enumerate(heads):
        closing = heads[r + 1] if r + 1 < len(heads) else n
        known = g[h] < len(table)
        geometry = table[g[h]] if known else (0, 0, 0)
        out.append(dict(count=int(geometry[0]), first=int(geometry[1]), vertex_offset=int(geometry[2]),
                        instance_count=int(first[closing]) - int(first[h]) if known else 0, first_instance=int(first[h]), draw=h))
    return out


def expected(fetched, starts, bases, ids, table, dtype, merge=False, region=0, capacity=None, pattern=None):
    """(bytes [rows, stride], command_counts) a command emission must leave in a target that held `pattern` (uint8 [rows, stride]),
    of which the first `capacity` positions (None: all rows) are the target's capacity.
    fetched: the results of the listed views in the emission's order (GpuVisibility.fetch(order="raw")); starts: the emission's
    starts[views + 1]; bases: None after emit_instances, (first_instance, draw_starts) of draw_bases() after a draw emission."""
    stride = dtype.itemsize
    per_view = []
    for v, f in enumerate(fetched):
        n = int(f["draw_count"])
        slots = f["visible_idx"][:n]
        if bases is None:
            first = [int(starts[v]) + k for k in range(n)] + [int(starts[v + 1])]
        else:
            first_instance, draw_starts = bases
            first = [int(first_instance[int(draw_starts[v]) + k]) for k in range(n)] + [int(starts[v + 1])]
        per_view.append(view_commands(slots, first, ids, table, merge))
    counts = np.array([len(c) for c in per_view], np.uint32)
    placed = {}  # position -> command dict, or None for an all-zero padding command
    at = 0
    for v, commands in enumerate(per_view):
        if region:
            for j in range(region):
                placed[v * region + j] = commands[j] if j < len(commands) else None
        else:
            for j, c in enumerate(commands):
                placed[at + j] = c
            at += len(commands)
    rows = len(pattern)
    room = rows if capacity is None else capacity
    out = pattern.copy()
    one = np.zeros(1, dtype)
    for position, c in placed.items():
        if position >= room:
            continue
        assert position < rows, "the pattern is too small for the test's own target"
        one[:] = 0
        if c is not None:
            for name in dtype.names:
                one[name] = c[name]
        out[position] = one.view(np.uint8).reshape(stride)
    return out, counts
