"""tools/ubench/score_exp.py [LIB]: kernel times of one forward-backward pass of the bench workload (SM = score mode, default 6) with the library LIB
(default: the built one)."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from htk_amd import capi, synth
if len(sys.argv) > 1:
    capi.LIBPATH = os.path.abspath(sys.argv[1])
s = synth.generate_fast(5000, 16, 6000, 1250, 500, seed=1000, model_seed=3)
model = capi.Model(s.packed()); accs = capi.Accs(model); fb = capi.ForwardBackward(model)
cfg = capi.fb_config(scoreMode=int(os.environ.get("SM", "6")))
X = np.concatenate(s.feats)
frameOff = capi.offsets([f.shape[0] for f in s.feats])
labOff = capi.offsets([len(q) for q in s.seqs])
labs = np.concatenate(s.seqs).astype(np.int32)
dX = capi.DevArray(X)
kt = np.zeros(4)
for it in range(7):
    accs.zero(None); fb.prepare(dX.ptr.value, frameOff, labOff, labs, None); fb.execute(cfg, accs, None); pr, st = fb.results(None)
    if it >= 2: kt += np.array(fb.kernel_times()[:4])
print(sys.argv[1:] , "kernels ms", [round(x / 5 * 1e3, 3) for x in kt], "sum pr %.6f ok %d" % (pr[st == 0].sum(), (st == 0).sum()))

