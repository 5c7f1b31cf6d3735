"""The range plan of telr_map (telr_amd/csrc/range_plan.h) through its tap, telr_debug_map_plan: pure host arithmetic on read lengths,
so the thresholds that only calls of hundreds of Mbp reach are pinned here without a device.  Every expectation is a literal worked
out by hand from the rules as telr_map stated them before the plan became a function (the derivation stands beside each case);
none comes from the function under test or from a re-statement of it."""
import contextlib
import os

import numpy as np
import pytest

from telr_amd.aligner import Engine

ENV = ("TELR_BATCH_MBP", "TELR_BATCH_KBP", "TELR_PIPELINE")
MI = 1 << 20
ONE = 1600 * MI                # 1,677,721,600: the range size when nothing cuts it


@contextlib.contextmanager
def environment(**kv):
    saved = {k: os.environ.get(k) for k in ENV}
    try:
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update({k: str(v) for k, v in kv.items()})
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def reads(n, length):
    return np.full(n, length, np.int32)


def edge_640(last):
    """5,000 reads: 4,999 of 134,217 (670,950,783 bases) and one of `last`"""
    a = reads(5000, 134217)
    a[-1] = last
    return a


# per_base 0.25 unless a case says otherwise: 0.8e9 / 0.25 = 3.2e9 leaves the cap at 1400 Mi = 1,468,006,400, and 1.6e9 / 0.25 = 6.4e9
# leaves "more than one range" at 1600 Mi
CASES = [
    # -- the four anchor cases ---------------------------------------------------------------------------------------------------
    # 500,000,000 bases: not above 1600 Mi, below 640 Mi = 671,088,640, no force -> one at a time, one range
    ("500Mbp", reads(5000, 100000), {}, {}, ("serial", ONE, [5000])),
    # 700,000,000 >= 640 Mi: nr = max(2, ceil(7e8 / 1,468,006,400) = 1) = 2; 350,000,000 + 140,000 + 1; 2,501 x 140,000 = 350,140,000 fits
    ("700Mbp", reads(5000, 140000), {}, {}, ("two_in_flight", 350140001, [2501, 5000])),
    # 4e9: ceil(4e9 / 1,468,006,400) = 3, made even 4; 1e9 + 200,000 + 1; 5,001 x 200,000 = 1,000,200,000 fits -> 5001, 5001, 5001, 4997
    ("4Gbp", reads(20000, 200000), {}, {}, ("two_in_flight", 1000200001, [5001, 10002, 15003, 20000])),
    # 2.5e9: ceil(2.5e9 / 1,468,006,400) = 2; 1.25e9 + 200,001; 6,251 x 200,000 = 1,250,200,000 fits
    ("2.5Gbp", reads(12500, 200000), {}, {}, ("two_in_flight", 1250200001, [6251, 12500])),
    # ... with sub-read voting the cap is 1100 Mi = 1,153,433,600: ceil(2.5e9 / that) = 3, made even 4; 625,000,000 + 200,001; 3,126 reads fit
    ("2.5Gbp vote", reads(12500, 200000), {"vote": True}, {}, ("two_in_flight", 625200001, [3126, 6252, 9378, 12500])),
    # -- 640 Mbp, to the base ----------------------------------------------------------------------------------------------------
    # 670,950,783 + 137,856 = 671,088,639: one short
    ("640Mi-1", edge_640(137856), {}, {}, ("serial", ONE, [5000])),
    # 671,088,640: 2 ranges of 335,544,320 + 137,857 + 1 = 335,682,178; 2,501 x 134,217 = 335,676,717 fits, 2,502 do not; the rest is 335,411,923
    ("640Mi", edge_640(137857), {}, {}, ("two_in_flight", 335682178, [2501, 5000])),
    # -- 4,000 queries -----------------------------------------------------------------------------------------------------------
    # 799,800,000 bases in 3,999 reads: large enough, too few reads
    ("3999 reads", reads(3999, 200000), {}, {}, ("serial", ONE, [3999])),
    # 4,000 reads, 8e8: 2 ranges of 4e8 + 200,001; 2,001 x 200,000 = 400,200,000 fits
    ("4000 reads", reads(4000, 200000), {}, {}, ("two_in_flight", 400200001, [2001, 4000])),
    # -- debug and pipe_nomem switch pipelining off (the 700-Mbp case) ----------------------------------------------------------------
    ("debug", reads(5000, 140000), {"debug": 1}, {}, ("serial", ONE, [5000])),
    ("pipe_nomem", reads(5000, 140000), {"pipe_nomem": True}, {}, ("serial", ONE, [5000])),
    # force overrides debug, not pipe_nomem
    ("debug force", reads(5000, 140000), {"debug": 1}, {"TELR_PIPELINE": "force"}, ("two_in_flight", 350140001, [2501, 5000])),
    ("pipe_nomem force", reads(5000, 140000), {"pipe_nomem": True}, {"TELR_PIPELINE": "force"}, ("serial", ONE, [5000])),
    # -- per-query targets: the same ranges, in turn; forced: two in flight; a call within one range: nothing to take turns ----------------
    ("qtarget", reads(5000, 140000), {"qtarget": True}, {}, ("in_turn", 350140001, [2501, 5000])),
    ("qtarget force", reads(5000, 140000), {"qtarget": True}, {"TELR_PIPELINE": "force"}, ("two_in_flight", 350140001, [2501, 5000])),
    ("qtarget 500Mbp", reads(5000, 100000), {"qtarget": True}, {}, ("serial", ONE, [5000])),
    # -- TELR_PIPELINE -----------------------------------------------------------------------------------------------------------
    ("pipeline=1", reads(5000, 140000), {}, {"TELR_PIPELINE": "1"}, ("serial", ONE, [5000])),
    ("pipeline=2", reads(5000, 140000), {}, {"TELR_PIPELINE": "2"}, ("two_in_flight", 350140001, [2501, 5000])),
    # =2 is the default, not force: fewer than 4,000 reads still run one at a time
    ("pipeline=2 3999", reads(3999, 200000), {}, {"TELR_PIPELINE": "2"}, ("serial", ONE, [3999])),
    # force: 3,999 reads, 799,800,000: 2 ranges of 399,900,000 + 200,001; 2,000 x 200,000 = 4e8 fits, 2,001 x do not
    ("force 3999", reads(3999, 200000), {}, {"TELR_PIPELINE": "force"}, ("two_in_flight", 400100001, [2000, 3999])),
    # force splits any call: 10,000 bases: 2 ranges of 5,000 + 1,000 + 1; 6 reads fit
    ("force tiny", reads(10, 1000), {}, {"TELR_PIPELINE": "force"}, ("two_in_flight", 6001, [6, 10])),
    # -- a range size from the environment: fixed, the plain greedy cut ------------------------------------------------------------------
    # 60 Ki = 61,440: 6 reads of 10,000 a range, 16 full ranges and 4 reads; fewer than 4,000 reads
    ("kbp", reads(100, 10000), {}, {"TELR_BATCH_KBP": "60"}, ("serial", 61440, list(range(6, 100, 6)) + [100])),
    ("kbp force", reads(100, 10000), {}, {"TELR_BATCH_KBP": "60", "TELR_PIPELINE": "force"}, ("two_in_flight", 61440, list(range(6, 100, 6)) + [100])),
    # a single range has nothing to pipeline, forced or not: 2,000 Ki = 2,048,000 holds the 1,000,000 bases
    ("kbp force one range", reads(100, 10000), {}, {"TELR_BATCH_KBP": "2000", "TELR_PIPELINE": "force"}, ("serial", 2048000, [100])),
    # 1 Mi = 1,048,576: 104 reads of 10,000 a range
    ("mbp", reads(300, 10000), {}, {"TELR_BATCH_MBP": "1"}, ("serial", 1048576, [104, 208, 300])),
    # 5,000 reads: pipelined by default; 48 full ranges end at 4,992; no density, no even count, no slack on a fixed size
    ("mbp 5000", reads(5000, 10000), {"per_base": 8.0}, {"TELR_BATCH_MBP": "1"}, ("two_in_flight", 1048576, list(range(104, 5000, 104)) + [5000])),
    # both set: TELR_BATCH_KBP is read last
    ("mbp+kbp", reads(100, 10000), {}, {"TELR_BATCH_MBP": "1", "TELR_BATCH_KBP": "60"}, ("serial", 61440, list(range(6, 100, 6)) + [100])),
    # -- the anchor density --------------------------------------------------------------------------------------------------------
    # unknown (0): no density term anywhere; the 700-Mbp case as it was
    ("density unknown", reads(5000, 140000), {"per_base": 0.0}, {}, ("two_in_flight", 350140001, [2501, 5000])),
    # 2 per base: cap 0.8e9 / 2 = 4e8 (1e9 bases: 2 ranges at the 1400-Mi cap); ceil(1e9 / 4e8) = 3, made even 4; 250,000,000 + 200,001; 1,251 reads fit
    ("density cap", reads(5000, 200000), {"per_base": 2.0}, {}, ("two_in_flight", 250200001, [1251, 2502, 3753, 5000])),
    # 8 per base: 0.8e9 / 8 = 1e8 is held at 256 Mi = 268,435,456 (1e8 would give 12 ranges): ceil(1.2e9 / 268,435,456) = 5, made even 6;
    # 200,000,000 + 240,001; 834 x 240,000 = 200,160,000 fits, 835 x do not; the last range holds 830
    ("density floor", reads(5000, 240000), {"per_base": 8.0}, {}, ("two_in_flight", 200240001, [834, 1668, 2502, 3336, 4170, 5000])),
    # 650,000,000 is below 640 Mi, but above the 1.6e9 / 3 = 533,333,333 bases that bring one range's anchors: cap max(256 Mi, 266,666,666);
    # ceil(6.5e8 / 268,435,456) = 3, made even 4; 162,500,000 + 130,001; 1,251 x 130,000 = 162,630,000 fits
    ("density splits", reads(5000, 130000), {"per_base": 3.0}, {}, ("two_in_flight", 162630001, [1251, 2502, 3753, 5000])),
    # -- the greedy cut ------------------------------------------------------------------------------------------------------------
    # a read longer than the limit is a range of its own
    ("long read", np.array([10000, 100000, 10000, 10000], np.int32), {}, {"TELR_BATCH_KBP": "60"}, ("serial", 61440, [1, 2, 4])),
    # empty reads ride along: 30,000 + 30,000 + 1,440 = 61,440 fits with the empty ones around it, the next base does not
    ("empty reads", np.array([0, 0, 30000, 0, 30000, 0, 1440, 0, 1, 0], np.int32), {}, {"TELR_BATCH_KBP": "60"}, ("serial", 61440, [8, 10])),
    ("all empty", np.zeros(5, np.int32), {}, {"TELR_BATCH_KBP": "60"}, ("serial", 61440, [5])),
    ("n=0", np.zeros(0, np.int32), {}, {}, ("serial", ONE, [])),
    # forced: 2 "ranges" of (0 + 1) / 2 + 0 + 1 = 1 base, and no read to put in them
    ("n=0 force", np.zeros(0, np.int32), {}, {"TELR_PIPELINE": "force"}, ("serial", 1, [])),
]


@pytest.mark.parametrize("name,lengths,args,env,want", CASES, ids=[c[0] for c in CASES])
def test_plan(name, lengths, args, env, want):
    args = dict({"per_base": 0.25}, **args)
    before = {k: os.environ.get(k) for k in ENV}
    with environment(**env):
        got = Engine.map_plan(lengths, **args)
    assert got == want
    assert {k: os.environ.get(k) for k in ENV} == before


def test_environment_is_read_per_call():
    """the tests of the executors set these in-process: a value read once per process would pin the first one seen"""
    a = reads(100, 10000)
    with environment(TELR_BATCH_KBP="60"):
        assert Engine.map_plan(a)[1] == 61440
    with environment(TELR_BATCH_KBP="30"):
        assert Engine.map_plan(a) == ("serial", 30720, list(range(3, 100, 3)) + [100])
    with environment():
        assert Engine.map_plan(a) == ("serial", ONE, [100])
