"""Child process of tests/test_screen_gpu.py and tests/test_screen_geometry_gpu.py: builds the screen's set from `ref` under the
environment it was started with (the prefilter switch is read when a set is finalized) and writes the hits of the packed reads and
the filter form that ran.  An `order` in the input is the processing order of the call.  `more` = k asks for k further calls on the
same context and set, each with its own plane_i, offsets_i, lengths_i and, where present, order_i (i = 0 .. k - 1): their hits go to
"more", a list of lists.
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

    def call(tag):
        order = d["order" + tag] if "order" + tag in d.files else None
        return [int(h) for h in ctx.screen_hits(d["plane" + tag], d["offsets" + tag], d["lengths" + tag], ks, order=order)]
    hits = call("")
    out = {"hits": hits, "filter": ctx.last_screen_filter(), "set_size": len(ks)}
    if "more" in d.files:
        out["more"] = [call("_%d" % i) for i in range(int(d["more"]))]
        out["filter_more"] = ctx.last_screen_filter()
    ks.close()
    ctx.close()
    with open(dst, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
