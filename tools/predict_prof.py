"""One warm train, one index build and PROF_REPS predicts of the training set
(for rocprofv3 --kernel-trace --stats runs; tools/kstats.py prints the table).

  rocprofv3 --kernel-trace --stats -d out -o predict -- python tools/predict_prof.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pypardis_amd import DBSCAN, synth

n = int(os.environ.get("PROF_N", "100000000"))
name = os.environ.get("PROF_CFG", "C2")
X, cfg = synth.make_config(name, n=n)
Xd = torch.from_numpy(X).cuda()
del X
m = DBSCAN(eps=cfg["eps"], min_samples=cfg["min_samples"],
           max_partitions=cfg.get("max_partitions") or 1).train(Xd)
for _ in range(int(os.environ.get("PROF_REPS", "3"))):
    out = m.predict(Xd)
torch.cuda.synchronize()
print("clusters", m.n_clusters_, "predict == labels_", bool(torch.equal(out, m.labels_)))
