"""minimap2's chaining scan (TELR_MF_CHAIN_SKIP, the oracle's 0x1000) without a GPU: the restatement of tests/chain_scan_ref.py
equals the oracle's f / p on every preset, on a per-target call and on hard-genome reads (it is the reference the hand-built GPU
cases are held to), the hand-built edges come out as worked out by hand, and the Python surface sets exactly the bit."""
import numpy as np
import pytest

from telr_amd import synth
from telr_amd.fasta import read_fasta
from telr_amd.presets import preset
from telr_amd._abi import MF_CHAIN_SKIP, MF_PER_TARGET, MapOpt
from telr_amd.cli_mm2 import parse_argv
import chain_scan_ref as R


def _check(targets, queries, pname, flags=0, qtarget=None, stats=None):
    from oracle import binding as ob
    io, mo = preset(pname, chain_skip=True)
    mo.flags |= flags
    oix = ob.OracleIndex([bytes(t).decode() if not isinstance(t, str) else t for t in targets], io)
    o = oix.map([bytes(q).decode() if not isinstance(q, str) else q for q in queries], mo, qtarget=qtarget, debug=True)
    f, p = R.chain_scan_all(o["anchors"], o["anchor_off"], mo, stats)
    np.testing.assert_array_equal(f, o["f"])
    np.testing.assert_array_equal(p, o["p"])
    return o


@pytest.mark.parametrize("pname", ["map-ont", "map-pb", "ngmlr-ont", "ngmlr-pacbio", "asm10"])
def test_restatement_equals_oracle_on_every_preset(data_dir, pname):
    _, ts = read_fasta(data_dir + "/ref_38kb.fasta")
    _, qs = read_fasta(data_dir + "/reads.fasta")
    o = _check(ts, qs, pname)
    assert len(o["anchors"]) > 500


def test_restatement_equals_oracle_per_target_call(data_dir):
    _, lib = read_fasta(data_dir + "/library.fasta")
    _, qs = read_fasta(data_dir + "/reads.fasta")
    _check(qs, lib, "asm10", flags=MF_PER_TARGET)
    # and a call with one target per query (qtarget)
    _, ts = read_fasta(data_dir + "/ref_38kb.fasta")
    _check(ts, qs[:6], "map-ont", qtarget=np.zeros(6, np.int32))


def test_restatement_equals_oracle_on_hard_genome_reads():
    d = synth.make_stage1_dataset(hard=True, seed=3, genome_len=2_000_000, n_reads=200, total_bases=1_800_000, n_ins=40)
    buf, off, ln = d["reads"]
    reads = [buf[off[i]:off[i] + ln[i]] for i in range(40)]
    st = {}
    _check([d["ref"]], reads, "map-ont", stats=st)
    assert st["breaks"] > 0 and st["max_link"] > 64


def test_hand_built_edges():
    mo = R.hand_opts()
    names = []
    for name, lists, checks in R.hand_cases():
        names.append(name)
        for q, exp in checks.items():
            f, p = R.chain_scan(lists[q], mo)
            for i, want in exp.items():
                assert p[i] == want, (name, q, i, p[i])
    assert len(names) >= 10


def test_hand_built_edges_worked_by_hand():
    """the numbers behind the three skip cases: C_m scores 15 + 10 (m - 1) - 31 through I, X_59 605 - 31, Z 502 - 6"""
    mo = R.hand_opts()
    f, p = R.chain_scan(R._skip_edge(26), mo)
    assert (f[-1], p[-1]) == (574, 59)
    f, p = R.chain_scan(R._skip_edge(27), mo)
    assert (f[-1], p[-1]) == (15 + 260 - 31, len(f) - 2)
    k = R._skip_edge(27, z=True)
    f, p = R.chain_scan(k, mo)
    zi = k.index(R.key(1715, 1515))
    assert (f[zi], p[zi]) == (502, 51) and (f[-1], p[-1]) == (574, 59)
    # the scan's own bookkeeping against a step-by-step walk of the oracle's loop on the 27-chain
    a = np.array(R._skip_edge(27), np.uint64)
    i = len(a) - 1
    sc = R.chain_scores(a[i], a[:i][::-1], mo)
    assert (sc[:27] == -31).all() and (sc[27:] == -31).all()


def test_restatement_small_lists_by_brute_force():
    """the vectorised restatement against a literal transcription of the oracle's loop on random lists"""
    mo = R.hand_opts()

    def literal(a):
        n = len(a); f = [0] * n; p = [-1] * n; t = [-1] * n; st = 0
        rev = [int(x) >> 63 for x in a]; g = [(int(x) >> 32) & 0x7fffffff for x in a]
        for i in range(n):
            while st < i and (rev[st] != rev[i] or g[i] - g[st] > mo.max_gap):
                st += 1
            if i - st > R.MAX_ITER:
                st = i - R.MAX_ITER
            best, bp, ns = int(a[i]) & 0xff, -1, 0
            for j in range(i - 1, st - 1, -1):
                sc = int(R.chain_scores(a[i], [a[j]], mo)[0])
                if sc == R.INT32_MIN:
                    continue
                v = f[j] + sc
                if v > best:
                    best, bp = v, j
                    ns = max(0, ns - 1)
                elif t[j] == i:
                    ns += 1
                    if ns > R.MAX_SKIP:
                        break
                if p[j] >= 0:
                    t[p[j]] = i
            f[i], p[i] = best, bp
        return f, p

    for L in R.random_lists(5, nq=6, lo=0, hi=300):
        f, p = R.chain_scan(L, mo)
        ef, ep = literal(np.array(L, np.uint64))
        assert list(f) == ef and list(p) == ep


def test_preset_chain_skip_sets_exactly_the_bit():
    for name in ("map-ont", "map-pb", "ngmlr-ont", "ngmlr-pacbio", "asm10"):
        io0, mo0 = preset(name)
        io1, mo1 = preset(name, chain_skip=True)
        assert not (mo0.flags & MF_CHAIN_SKIP)
        assert mo1.flags == mo0.flags | MF_CHAIN_SKIP
        for fld, _ in MapOpt._fields_:
            if fld != "flags":
                assert getattr(mo0, fld) == getattr(mo1, fld), (name, fld)
    assert MF_CHAIN_SKIP == 0x1000


def test_cli_max_chain_skip_and_iter():
    base = ["minimap2", "--cs", "--MD", "-Y", "-L", "-ax", "map-ont"]
    for extra in (["--max-chain-skip", "25"], ["--max-chain-iter", "5000"], ["--max-chain-skip=25", "--max-chain-iter=5000"]):
        o = parse_argv(base + extra + ["ref.fa", "reads.fa"])
        assert o["chain_skip"] and (o["target"], o["query"]) == ("ref.fa", "reads.fa") and o["preset"] == "map-ont"
    for extra in (["--max-chain-skip", "26"], ["--max-chain-iter", "2000"], ["--max-chain-skip=0"], ["--max-chain-iter"]):
        with pytest.raises(SystemExit):
            parse_argv(base + extra + ["ref.fa", "reads.fa"])


def test_reference_argv_shapes_are_unchanged():
    shapes = [
        ["ngmlr", "-r", "ref.fa", "-q", "reads.fa", "-x", "ont", "-t", "8", "--rg-id", "S", "--rg-sm", "S", "--rg-lb", "ont", "--no-progress"],
        ["minimap2", "--cs", "--MD", "-Y", "-L", "-ax", "map-pb", "ref.fa", "reads.fa"],
        ["minimap2", "-t", "1", "-ax", "map-ont", "-r2k", "cns.fa", "reads.fa"],
        ["minimap2", "-cx", "map-ont", "--secondary=no", "-v", "0", "subj.fa", "qry.fa"],
        ["minimap2", "-cx", "map-pb", "contig.fa", "lib.fa", "-v", "0", "-t", "4"],
        ["minimap2", "-a", "-x", "map-ont", "-v", "0", "contig.fa", "reads.fa"],
        ["minimap2", "-cx", "asm10", "-v", "0", "-N", "10", "ref.fa", "flank.fa"],
    ]
    for a in shapes:
        o = parse_argv(a)
        assert o.pop("chain_skip") is False
        assert set(o) == {"tool", "preset", "sam", "cigar", "md", "cs", "softclip", "secondary", "best_n", "bw", "target", "query", "rg", "threads"}
