"""Host-side check of the one table builder behind the optimizer / spectral-norm kernels (OptTables, csrc/sgv_ew.h +
csrc/opt_tables.hip).  tests/opt_tables_host.hip builds the tables over a host buffer and prints them; the geometry formulas of
sgv_ew.h are restated here.  No GPU: the construction layer makes no HIP call."""
import os
import shutil
import subprocess
from collections import Counter

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not HIPCC, reason="hipcc not found: the table builder's stand-alone program cannot be compiled")

N_GROUPS = 3
# (taps, rows, cols, active, tiled, group, copy); rows = 0: a plain tensor of `cols` elements.  The smallest geometries at which every
# chunking rule has a remainder and more than one block: [3, 65, 68] crosses the 64-row item, the 64 x 64 tile, the 32 x 32 copy tile and
# the 64-element sum chunk, [1, 8, 1028] the 1024-column item, n = 8196 the 8192-element flat chunk.  Groups are interleaved so that the
# sort by group has something to move.
ENTRIES = [
    (1, 4, 4, 1, 0, 2, 0),
    (3, 65, 68, 1, 1, 0, 1),
    (1, 8, 1028, 1, 0, 1, 1),
    (0, 0, 8196, 1, 0, 2, 0),
    (3, 65, 68, 0, 0, 0, 0),       # inactive, <G,W> still from the flat pass
    (1, 8, 1028, 1, 1, 1, 0),
    (0, 0, 8196, 1, 0, 0, 0),
    (1, 4, 4, 1, 0, 0, 0),
    (3, 65, 68, 1, 0, 1, 1),
]


def cdiv(a, b):
    return (a + b - 1) // b


def al4(n):
    return cdiv(n, 4) * 4


# sgv_ew.h: OPT_CHUNK 8192, SN_ROWS_PER_ITEM 64, SN_COLS_PER_ITEM 1024, SN_SUM_CHUNK 64, OPT_TILE 64, COPY_TILE 32
def gemv_items(t, r, c): return t * cdiv(r, 64) * cdiv(c, 1024)
def tsum_items(t, c): return cdiv(t * c, 64)
def ssum_items(r): return cdiv(r, 64)
def flat_items(n): return cdiv(n, 8192)
def tile_items(t, r, c): return t * cdiv(r, 64) * cdiv(c, 64)
def copy_items(t, r, c): return t * cdiv(r, 32) * cdiv(c, 32)
def scratch_blocks(t, r, c): return [t * c, r, cdiv(r, 64) * t * c, t * cdiv(c, 1024) * r]      # tmp_t, tmp_s, tpart, spart


def numel(e):
    return e[0] * e[1] * e[2] if e[1] else e[2]


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("opt_tables") / "opt_tables_host")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", os.path.join(HERE, "opt_tables_host.hip"), "-o", exe],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([exe, str(N_GROUPS)] + [",".join(map(str, e)) for e in ENTRIES], check=True, capture_output=True, text=True).stdout
    t = dict(sn={}, adam={}, items={}, off={}, fin=[], scratch=None)
    for line in out.splitlines():
        w = line.split()
        if w[0] == "sn":
            t["sn"][int(w[1])] = dict(entry=int(w[3]), scratch=[int(x) for x in w[5:9]])
        elif w[0] == "adam":
            t["adam"][int(w[1])] = dict(entry=int(w[3]), sn=int(w[5]))
        elif w[0] == "item":
            t["items"].setdefault(w[1], []).append((int(w[2]), int(w[3])))
        elif w[0] == "off":
            t["off"][w[1]] = [int(x) for x in w[2:]]
        elif w[0] == "fin":
            t["fin"].append(dict(entry=int(w[2]), src=int(w[4]), count=int(w[6])))
        elif w[0] == "scratch":
            t["scratch"] = dict(base_mod16=int(w[2]), end=int(w[4]), total=int(w[6]))
    for name in ("sn", "sn_unf", "tsum", "ssum", "dot", "adam", "flat", "tile", "copy"):
        t["items"].setdefault(name, [])
    return t


def expected_counts(tables):
    """list name -> {descriptor: item count} from the formulas"""
    exp = {k: {} for k in tables["items"]}
    for si, d in tables["sn"].items():
        t, r, c, active, tiled, _, _ = ENTRIES[d["entry"]]
        if active:
            exp["sn"][si] = gemv_items(t, r, c)
            exp["tsum"][si] = tsum_items(t, c)
            exp["ssum"][si] = ssum_items(r)
            if not tiled:
                exp["sn_unf"][si] = gemv_items(t, r, c)
        if not tiled:
            exp["dot"][si] = flat_items(t * r * c)
    for ai, a in tables["adam"].items():
        e = ENTRIES[a["entry"]]
        exp["adam"][ai] = flat_items(numel(e))
        if e[4]:
            exp["tile"][ai] = tile_items(e[0], e[1], e[2])
        else:
            exp["flat"][ai] = flat_items(numel(e))
        if e[6]:
            exp["copy"][ai] = copy_items(e[0], e[1], e[2]) if e[1] else copy_items(1, 1, e[2])
    return exp


def test_descriptors_follow_insertion_order(tables):
    assert [a["entry"] for _, a in sorted(tables["adam"].items())] == list(range(len(ENTRIES)))
    sn_entries = [i for i, e in enumerate(ENTRIES) if e[1]]
    assert [d["entry"] for _, d in sorted(tables["sn"].items())] == sn_entries
    for a in tables["adam"].values():
        assert (a["sn"] >= 0) == bool(ENTRIES[a["entry"]][1])
        if a["sn"] >= 0:
            assert tables["sn"][a["sn"]]["entry"] == a["entry"]


def test_every_chunk_once_with_the_formula_count(tables):
    exp = expected_counts(tables)
    for name, items in tables["items"].items():
        assert len(set(items)) == len(items), f"{name}: a (desc, chunk) pair occurs twice"
        want = {(d, c) for d, n in exp[name].items() for c in range(n)}
        assert set(items) == want, f"{name}: items differ from the formula"
    assert any(n > 1 for n in exp["sn"].values()) and any(n > 1 for n in exp["flat"].values())      # the cases do cross a chunk


def test_inactive_and_tiled_rules(tables):
    inactive = {si for si, d in tables["sn"].items() if not ENTRIES[d["entry"]][3]}
    assert inactive
    for name in ("sn", "sn_unf", "tsum", "ssum"):
        assert not inactive & {d for d, _ in tables["items"][name]}
    tiled_sn = {si for si, d in tables["sn"].items() if ENTRIES[d["entry"]][4]}
    tiled_adam = {ai for ai, a in tables["adam"].items() if ENTRIES[a["entry"]][4]}
    assert tiled_sn and tiled_adam
    assert not tiled_sn & {d for d, _ in tables["items"]["sn_unf"]}
    assert not tiled_sn & {d for d, _ in tables["items"]["dot"]}
    assert not tiled_adam & {d for d, _ in tables["items"]["flat"]}
    assert {d for d, _ in tables["items"]["tile"]} == tiled_adam


def test_plain_lists_keep_insertion_order(tables):
    for name in ("sn", "sn_unf", "tsum", "ssum", "adam", "copy"):
        items = tables["items"][name]
        assert items == sorted(items), name      # descriptors in insertion order, chunks ascending


@pytest.mark.parametrize("name,which", [("dot", "sn"), ("flat", "adam"), ("tile", "adam")])
def test_group_offsets_and_order_within_a_group(tables, name, which):
    items, off = tables["items"][name], tables["off"][name]
    assert len(off) == N_GROUPS + 1 and off[0] == 0 and off[-1] == len(items)
    assert all(a <= b for a, b in zip(off, off[1:]))
    group_of = {k: ENTRIES[d["entry"]][5] for k, d in tables[which].items()}
    used = set()
    for g in range(N_GROUPS):
        part = items[off[g]:off[g + 1]]
        assert all(group_of[d] == g for d, _ in part)
        assert part == sorted(part)          # insertion order of the descriptors, chunks ascending
        used |= {g} if part else set()
    assert len(used) >= 2                    # the sort had something to do


def test_fin_dots_tile_the_dot_list(tables):
    fin, off, items = tables["fin"], tables["off"]["fin"], tables["items"]["dot"]
    assert len(off) == N_GROUPS + 1 and off[0] == 0 and off[-1] == len(fin)
    assert all(a <= b for a, b in zip(off, off[1:]))
    pos = 0
    for i, f in enumerate(fin):
        assert f["src"] == pos, "gap or overlap in front of FinDot %d" % i
        si = next(k for k, d in tables["sn"].items() if d["entry"] == f["entry"])
        assert items[pos:pos + f["count"]] == [(si, c) for c in range(f["count"])]      # it sums its own descriptor's partials
        g = ENTRIES[f["entry"]][5]
        assert off[g] <= i < off[g + 1] and tables["off"]["dot"][g] <= pos < tables["off"]["dot"][g + 1]
        pos += f["count"]
    assert pos == len(items)
    assert Counter(f["entry"] for f in fin) == Counter(d["entry"] for d in tables["sn"].values() if not ENTRIES[d["entry"]][4])


def test_scratch_blocks_disjoint_aligned_and_exact(tables):
    s = tables["scratch"]
    assert s["base_mod16"] == 0
    spans, total = [], 0
    for d in tables["sn"].values():
        t, r, c = ENTRIES[d["entry"]][:3]
        sizes = scratch_blocks(t, r, c)
        total += sum(al4(n) for n in sizes)
        for o, n in zip(d["scratch"], sizes):
            assert o % 4 == 0                # 4 floats = 16 bytes from a 16-byte aligned base
            spans.append((o, o + n))
    spans.sort()
    assert spans[0][0] == 0
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert s["total"] == total and s["end"] == total and al4(spans[-1][1]) == total
