"""One rank of tests/test_gpu_summary.py::test_ranks_on_one_gpu: takes its block of the arrays in CASE.npz, joins the communicator
(id through a file, like the command line does) and summarises — collectively (host arrays, device pointers, lengths alone) and
on its own (global = 0 on the same context).
usage: _summary_worker.py RANK WORLD WORKDIR CASE"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from filtlong_amd import api  # noqa: E402

rank, world, work, case = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
d = np.load(os.path.join(work, case + ".npz"))
lo, hi = int(d["bounds"][rank]), int(d["bounds"][rank + 1])
ln, mq, wq, mask = (np.ascontiguousarray(d[k][lo:hi]) for k in ("length", "mean", "window", "mask"))
ctx = api.Context(0)  # every rank on the one GPU of the box: only the loopback communicator allows that
idf = os.path.join(work, case + ".id")
if rank == 0:
    uid = ctx.comm_unique_id()
    open(idf + ".tmp", "wb").write(uid)
    os.rename(idf + ".tmp", idf)
else:
    for _ in range(3000):
        if os.path.exists(idf):
            break
        time.sleep(0.01)
    uid = open(idf, "rb").read()
ctx.comm_init(uid, rank, world)
out = {"global": ctx.summary(ln, mq, wq, mask, global_=True)}
out["local"] = ctx.summary(ln, mq, wq, mask, global_=False)
import torch  # noqa: E402
dev = [torch.from_numpy(a).cuda() for a in (ln, mq, wq, mask)]
torch.cuda.synchronize()
out["global_dev"] = ctx.summary_dev(len(ln), *[t.data_ptr() if t.numel() else None for t in dev], global_=True)
out["global_lengths_only"] = ctx.summary(ln, global_=True)
json.dump(out, open(os.path.join(work, "%s.out%d.json" % (case, rank)), "w"))
ctx.comm_destroy()
ctx.close()
