"""The planted trace-back paths of tests/tb_paths.py, checked without a device: every path is the oracle's own optimal path (or on
the allow list of runs the ngmlr-* costs never take), the restated geometry agrees with the library's class table, every family
hits the edges it is aimed at, and the identity the derived mlen of d_traceback_rows rests on holds for the oracle's results."""
import numpy as np
import pytest

import dp_edges as de
import tb_paths as tp
from telr_amd.aligner import Engine


@pytest.fixture(scope="module")
def built():
    return tp.build()


def _cases(built, fam, name=None, cls=None):
    return [c for s, c in built.cases if c.want.fam == fam and (name is None or s == name) and (cls is None or c.want.cls == cls)]


def test_geometry_is_the_class_table():
    t = Engine.dp_class_table()
    col = {n: k for k, n in enumerate(Engine.DP_CLASS_COLUMNS)}
    for c, rb in tp.ROW_BYTES.items():
        assert rb == 4 * t[c, col["row_dwords"]], c
        assert (tp.LAYOUT[c] == tp.TILES) == bool(t[c, col["tiled"]]), c
    for c, rb in tp.NIBBLE_ROW_BYTES.items():
        assert rb == 4 * ((t[c, col["regs"]] + 1) // 2), c
    for c, l in tp.LANES.items():
        assert l == t[c, col["lanes"]], c
    for c, (lo, hi) in tp.D_RANGE.items():
        assert hi == t[c, col["maxd"]] == de.UPPER_D[c], c
    for c in tp.LAYOUT:
        assert (tp.LAYOUT[c] == tp.BYTES) == (t[c, col["row_dwords"]] == 0), c
    assert sorted(tp.ROW_BYTES[c] for c in tp.A_CLASSES) == [16, 20, 24, 28, 32, 40, 48, 64, 128]
    assert sorted(tp.NIBBLE_ROW_BYTES.values()) == [8, 12]
    assert {rb: tp.phase_period(rb) for rb in (8, 12, 16, 20, 24, 28, 32, 40, 48, 64, 128)} == \
        {8: 8, 12: 16, 16: 4, 20: 16, 24: 8, 28: 16, 32: 2, 40: 8, 48: 4, 64: 1, 128: 1}
    assert [de.d_onep_d(m.q, m.e, m.q2, m.e2) for m in (de._mo(n) for n in tp.AFFINE_SETS)] == [20, 20, 25]


def test_every_path_is_realised_or_on_the_allow_list(built):
    off = [(s, w.key) for s, w in built.dropped if not tp.allowed_drop(s, w)]
    assert not off, "not the oracle's path within %d seeds: %s" % (tp.SEEDS, off[:10])
    # what the ngmlr-ont costs drop is exactly the runs of one cell: 32 per class of family A, 16 per kind of the tiled class
    assert all(any(op == "M" and ln == 1 for op, ln in w.spec) for _, w in built.dropped)
    n = {}
    for s, w in built.dropped:
        n[(s, w.fam)] = n.get((s, w.fam), 0) + 1
    print("dropped (allow list):", n)
    assert n == {("ngmlr-ont", "A"): 32 * len(tp.A_CLASSES), ("ngmlr-ont", "C"): 32}
    # a path no band of its class holds is a gap run, never a run case
    assert all(w.what.startswith(("gap", "lowedge")) or w.cls == 4 for _, w in built.narrow)
    for s, c in built.cases:
        assert 0 <= c.seed < tp.SEEDS
        assert tp.dims(c.want.spec) == (c.prob.m, c.prob.n)


def _a_rowb(mo, lim, c):
    nib = not mo.cx_scale and c in tp.NIBBLE_BIT and bool(lim["tb4_mask"] & tp.NIBBLE_BIT[c])
    return (tp.NIBBLE_ROW_BYTES[c] if nib else tp.ROW_BYTES[c]), nib


@pytest.mark.parametrize("name", tp.A_SETS)
def test_family_a_hits_every_row_phase_and_trip_length(built, name):
    mo, lim = built.sets[name], built.lims[name]
    for c in tp.A_CLASSES:
        rowb, nib = _a_rowb(mo, lim, c)
        period = tp.phase_period(rowb)
        seen, trips, cut = set(), set(), False
        for x in _cases(built, "A", name, c):
            if not x.want.what.startswith("run"):
                continue
            (ln, i, j), = tp.inner_runs(x.want.spec)
            seen.add((((i + j) >> 1) % period, ln))
            tr, ct = tp.rows_trips(x.want.spec, x.dlo, rowb, nib, (ln, i, j))
            assert sum(tr) == ln
            trips |= set(tr)
            cut |= ct
        need = {(ph, r) for ph in range(period) for r in (1, 2, 3, 4, 5) if not (r == 1 and name.startswith("ngmlr"))}
        assert need <= seen, "class %d (%d-byte rows): missing %s" % (c, rowb, sorted(need - seen)[:8])
        assert {r for _, r in seen} >= {2, 3, 4, 5, 8, 9}
        # the longest trip the wave's two lines allow: a cell's room is at most 63 bytes, so rows of 64 and 128 bytes never give one
        assert max(trips) == min(4, 1 + 63 // rowb), (c, rowb, trips)
        assert cut, (c, rowb)           # and the room guard ended a trip that the run would have continued
        # first runs of 0 .. 4 cells in front of a gap (mij > k, and the boundary run when the path starts with the gap)
        leads = {x.want.what for x in _cases(built, "A", name, c) if x.want.what.startswith("lead")}
        want = {"lead%d%s" % (k, op) for k in range(5) for op in "ID"}
        assert want - leads <= {w.what for s, w in built.dropped if s == name and w.cls == c}, (c, want - leads)
        if name in tp.AFFINE_SETS:
            assert want <= leads


@pytest.mark.parametrize("name", tp.AFFINE_SETS)
def test_family_a_gap_runs_around_onep(built, name):
    mo = built.sets[name]
    onep = de.d_onep_d(mo.q, mo.e, mo.q2, mo.e2)
    want = {"gap%d%s%s" % (g, op, f) for g in (onep - 1, onep, onep + 1, 2 * onep) for op in "ID" for f in ("", " first")}
    for c in tp.A_CLASSES:
        got = {x.want.what for x in _cases(built, "A", name, c) if x.want.what.startswith("gap")}
        narrow = {w.what for s, w in built.narrow if s == name and w.cls == c}
        assert got | narrow == want and not got & narrow, c
        if tp.D_RANGE[c][1] >= 2 * onep + 2:
            assert got == want, c
    # both pieces are charged somewhere: a run the first piece pays and one the second pays, inside the path and as its first run
    for c in (16, 22):
        got = {x.want.what for x in _cases(built, "A", name, c)}
        assert want <= got


@pytest.mark.parametrize("name", tp.AFFINE_SETS)
def test_derived_mlen_identity_holds_for_the_oracle(built, name):
    """a ml - b (mc - ml) - gc = score with gc by the two-piece rule: what d_traceback_rows derives mlen from (nibble and tag8 cells).
    Every family-A case of the three affine sets; under ngmlr-ont's convex cost the walk reads plain flags and derives nothing"""
    mo = built.sets[name]
    lut = np.full(256, 4, np.int8)
    for k, ch in enumerate(b"ACGT"):
        lut[ch] = k
    n = 0
    for x in _cases(built, "A", name):
        ml, ci, cj = de.mlen_of(tp.cig_words(x.want.spec), lut[x.prob.A], lut[x.prob.B])
        mc = sum(ln for op, ln in x.want.spec if op == "M")
        assert (ci, cj) == (x.prob.m, x.prob.n)
        assert mo.a * ml - mo.b * (mc - ml) - tp.gap_cost(mo, x.want.spec) == x.score, x.want.key
        n += 1
    assert n > 2000


def test_family_a_encodings_and_waves(built):
    encs = {}
    for g in built.groups:
        if g.fam != "A":
            continue
        mo, lim = built.sets[g.set], built.lims[g.set]
        probs = g.probs()
        cs = [(de.expect_class(p.kind, p.dhi - p.dlo + 1, p.m + p.n, lim, False), p.m + p.n) for p in probs]
        cells = tp.wave_cells(mo, lim, cs)
        for c, e in cells.items():
            assert len(e) == 1, "%s / %s: class %d mixes %s" % (g.set, g.name, c, e)
            want = g.enc or ("cx" if mo.cx_scale else "nibble" if c in tp.NIBBLE_BIT else "tag8")
            assert e == {want}, (g.set, g.name, c, e)
            encs.setdefault((g.set, c), set()).update(e)
        if g.enc == "plain":
            (c,) = cells
            assert len(probs) == 64 // tp.LANES[c] and probs[0].m + probs[0].n == lim["tag8_steps"] + 1
        if g.name.startswith("waves of"):
            cnt = int(g.name.split()[-1])
            for c in tp.A_CLASSES:
                mine = [x for x in g.cases if x.want.cls == c]
                assert len(mine) == cnt and sum(x.want.what == "long" for x in mine) == 1, (g.set, g.name, c, len(mine))
                assert max(x.prob.m + x.prob.n for x in mine) > 2 * min(x.prob.m + x.prob.n for x in mine)      # lanes that finish early
    for name in tp.AFFINE_SETS:
        for c in tp.A_CLASSES:
            assert encs[(name, c)] == ({"nibble"} if c in tp.NIBBLE_BIT else {"tag8", "plain"}), (name, c, encs[(name, c)])
    assert all(encs[("ngmlr-ont", c)] == {"cx"} for c in tp.A_CLASSES)


def test_family_b_reaches_the_window_edges(built):
    by_layout = {}
    strides = set()
    for s, x in built.cases:
        if x.want.fam != "B":
            continue
        lay = tp.LAYOUT[x.want.cls]
        ev = tp.walk_w(x.want.spec, x.dlo, lay)
        assert sum(ev["trips"]) == sum(ln for op, ln in x.want.spec if op == "M")
        d = by_layout.setdefault(lay, dict(full=0, cut32=0, clamp=0, edge=0, gapI=0, gapD=0, maxtrip=0, classes=set(), runs={}))
        d["classes"].add(x.want.cls)
        for k in ("full", "cut32", "clamp", "edge"):
            d[k] += ev[k]
        if ev["reload_in_gap"] and x.want.what.startswith("gap"):
            d["gap" + x.want.what[-1]] += 1
        d["maxtrip"] = max(d["maxtrip"], max(ev["trips"]))
        if x.want.what.startswith("run"):
            d["runs"].setdefault(x.want.cls, set()).add(x.want.what)
        if lay == tp.BYTES:
            strides.add(((x.prob.dhi - x.prob.dlo + 3) // 2) % 4)
    print({k: {a: b for a, b in v.items() if a != "runs"} for k, v in by_layout.items()})
    assert by_layout[tp.LINES]["classes"] == {19, 20, 21} and by_layout[tp.REGROWS]["classes"] == {7, 8, 9} and by_layout[tp.BYTES]["classes"] == {1, 2, 4}
    allruns = {"run%d%s" % (r, o) for r in tp.B_RUNS for o in ("ID", "DI")}
    for lay, d in by_layout.items():
        for c, r in d["runs"].items():
            assert c == 4 or r == allruns, (c, allruns - r)
        # a full ballot where the layout's reach is 64 cells; the byte layout's is cut at 32
        if lay == tp.BYTES:
            assert d["full"] == 0 and d["cut32"] > 0 and d["maxtrip"] == 32
        else:
            assert d["full"] > 0 and d["maxtrip"] == 64
        assert d["gapI"] > 0 and d["gapD"] > 0, "%s: no window reload inside an open gap run (I %d, D %d)" % (lay, d["gapI"], d["gapD"])
        assert d["clamp"] > 0 and d["edge"] > 0, lay
    assert strides >= {1, 2, 3}, strides       # (D + 2) / 2 mod 4: the unaligned-row load of the byte layout


def test_family_c_starts_runs_on_every_row_of_a_tile(built):
    for c in (18, 23, 24):
        seen, trips = set(), set()
        for x in _cases(built, "C", cls=c):
            if x.want.what.startswith("run"):
                run, = tp.inner_runs(x.want.spec)
                kr, tr = tp.lane_trips(run)
                assert sum(tr) == run[0] and tr[0] == min(run[0], kr + 1, 4)
                seen.add((kr, run[0]))
                trips |= set(tr)
        assert {(kr, r) for kr in range(4) for r in (1, 2, 3, 4)} <= seen, (c, sorted(seen))
        assert trips == {1, 2, 3, 4}
        kinds = {x.prob.kind for x in _cases(built, "C", cls=c)}
        assert kinds == {1, 2}
        # a gap run that crosses a column group of the tile (sl >> 3)
        cross = 0
        for x in _cases(built, "C", cls=c):
            if x.want.what.startswith("gap"):
                e = tp.ends(x.want.spec)
                s0, s1 = ((e[k][3] - e[k][2] - x.dlo) >> 4 for k in (0, 1))
                cross += s0 != s1
        assert cross >= 2, c
    for c in (0, 5, 6):
        runs = {x.want.what for x in _cases(built, "C", cls=c) if x.want.what.startswith("run")}
        assert len(runs) == 5 * 2 * 8, (c, len(runs))


def test_family_d_holds_one_more_than_the_wave_walk_takes(built):
    seen = {}
    for g in built.groups:
        if g.fam != "D":
            continue
        lim = built.lims[g.set]
        cls = {de.expect_class(p.kind, p.dhi - p.dlo + 1, p.m + p.n, lim, bool((p.A == ord("N")).any())) for p in g.probs()}
        assert len(cls) == 1
        seen.setdefault(cls.pop(), []).append(len(g.probs()))
        assert all(150 <= p.m + p.n <= 260 for p in g.probs())
    assert seen == {19: [tp.TBW_MAX, tp.TBW_MAX + 1], 7: [tp.TBW_MAX, tp.TBW_MAX + 1], 1: [tp.TBW_MAX, tp.TBW_MAX + 1]}
