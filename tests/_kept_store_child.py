"""Child of tests/test_gpu_kept_store.py: a process that never creates an engine.  It loads the blob at argv[1] (Kept.load),
asks lh_kept_across for the percentiles argv[2:], and prints count, pkeys, pvalid and the values as one JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import loghisto_amd
    P = [float(x) for x in sys.argv[2:]]
    with loghisto_amd.Kept.load(sys.argv[1]) as k:
        got = k.across([], P, first=k.info["first"])
        print(json.dumps(dict(info=k.info, count=[int(x) for x in got["count"]], pkeys=got["pkeys"].tolist(),
                              pvalid=got["pvalid"].tolist(), pvals=[[repr(float(v)) for v in row] for row in got["pvals"]])))


if __name__ == "__main__":
    main()
