"""One engine run of every planted-path group of tests/tb_paths.py against the oracle, in a process of its own: the TELR_AB
switches that change the trace-back format (tb8, no_tag8) or send every class through the generic lane walk (tb_one_launch) are
read once per process.  Prints "tb paths ok: <problems> problems" or the mismatches."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tb_paths as tp

if __name__ == "__main__":
    import torch  # noqa: F401  (the engine binds to the HIP runtime torch loads)
    from telr_amd.aligner import Engine
    res = tp.run_all(Engine(0))
    print("\n".join(tp.summary(res)))
    bad = [b for _, b, _ in res.values() for b in b]
    total = sum(n for n, _, _ in res.values())
    if bad:
        print("\n".join(bad[:40]))
        print("tb paths FAILED: %d of %d problems" % (len(bad), total))
        sys.exit(1)
    print("tb paths ok: %d problems" % total)
