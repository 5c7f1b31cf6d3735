"""Times the cohort merge (Engine.merge_sites, telr_merge_sites) on a synthetic cohort: tests/cohort_ref.py's seeded
generator scaled up to 200 samples with about 1,000 calls each on a target table of dm6's size (its seven chromosome arms), 50 families.
Wall clock around the Python call -- validation, the upload of the entries, the kernels, the copy back --, median of 5 after one untimed
call; the plain-Python checker of the tests on the same input next to it, run once, and the two outputs asserted equal array for array.
The kernels alone are not timed.  Nothing asserts a time.  Writes profiles/cohort_merge_time.json.

    python tools/cohort_time.py [--samples 200] [--calls 1000] [--families 50] [--repeat 5] [--out profiles/cohort_merge_time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DM6 = (23513712, 25286936, 28110227, 32079331, 1348131, 23542271, 3667352)          # chr2L, 2R, 3L, 3R, 4, X, Y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--calls", type=int, default=1000, help="calls per sample, about")
    ap.add_argument("--families", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cohort_merge_time.json"))
    a = ap.parse_args()
    import numpy as np
    import cohort_ref as cref
    import torch  # noqa: F401
    from telr_amd.aligner import Engine
    from telr_amd._abi import COHORT_ENTRY_DTYPE
    # a locus is carried by a quarter of the samples on average (generate: Beta(0.5, 1.5)), so calls per sample = loci / 4
    entries = cref.generate(seed=a.seed, target_lens=DM6, n_groups=a.families, n_samples=a.samples, n_loci=4 * a.calls)
    e = np.array(entries, np.int32).view(COHORT_ENTRY_DTYPE).reshape(-1)
    eng = Engine(0)
    times, got = [], None
    for _ in range(a.repeat + 1):
        t0 = time.perf_counter()
        got = eng.merge_sites(e, len(DM6))
        times.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    want = cref.merge(entries)
    t_ref = time.perf_counter() - t0
    A = cref.arrays(want)
    for f in cref.SITE_FIELDS:
        assert np.array_equal(got.sites[f], A[f]), f
    for name in ("member_off", "members", "sample_off", "samples"):
        assert np.array_equal(getattr(got, name), A[name]), name
    flags = got.sites["flags"]
    out = {
        "samples": a.samples, "families": a.families, "targets": len(DM6), "target_bases": int(sum(DM6)), "entries": int(len(e)), "seed": a.seed,
        "sites": int(len(got.sites)), "shadowed": int((flags & 1 != 0).sum()), "crowded": int((flags & 2 != 0).sum()),
        "largest_cluster": int(got.sites["n_members"].max()), "device": eng.device_name(),
        "merge_sites_s_median": float(np.median(times[1:])), "merge_sites_s_all": times[1:], "merge_sites_s_first_call": times[0],
        "python_checker_s": t_ref, "outputs_equal": True,
        "timing": "wall clock around Engine.merge_sites (validation, upload, kernels, copy back; ends in a stream synchronisation), %d repeats after "
                  "one untimed call, same process; the checker (tests/cohort_ref.py: merge) once on the same entries; the kernels alone were not timed" % a.repeat,
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("entries", "sites", "shadowed", "crowded", "largest_cluster", "merge_sites_s_median", "merge_sites_s_all", "python_checker_s")}))
    eng.close()


if __name__ == "__main__":
    main()
