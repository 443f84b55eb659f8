"""Child process of tests/test_screen_gpu.py: builds the screen's set from `ref` under the environment it was started with (the
prefilter switch is read when a set is finalized) and writes the hits of the packed reads and the filter form that ran.
    python _screen_worker.py IN.npz OUT.json"""
import json
import sys

import numpy as np

from filtlong_amd import api


def main(src, dst):
    d = np.load(src)
    ctx = api.Context(0)
    ks = api.Kmers(ctx)
    ks.add_screen_fasta([d["ref"].tobytes()])
    ks.finalize()
    hits = ctx.screen_hits(d["plane"], d["offsets"], d["lengths"], ks)
    out = {"hits": [int(h) for h in hits], "filter": ctx.last_screen_filter(), "set_size": len(ks)}
    ks.close()
    ctx.close()
    with open(dst, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
