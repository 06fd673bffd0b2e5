"""Host wall-clock per call of the per-frame route ops at N = 1024: median of 2000 calls after 200 warm-up calls, one synchronise at the
end.  usage: op_args_host_time.py <tree root> <label>"""
import json
import os
import statistics
import sys
import time

root, label = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, root)
import numpy as np      # noqa: E402
import torch            # noqa: E402
from gspl_amd import ops  # noqa: E402

assert os.path.dirname(os.path.abspath(ops.__file__)).startswith(root), ops.__file__
DEV, N = "cuda:0", 1024
g = torch.Generator().manual_seed(0)


def R(*shape):
    return torch.rand(*shape, generator=g).to(DEV)


def cases():
    means, centre, dc, rest = R(N, 3), R(3), R(N, 1, 1), R(N, 15, 1)
    yield "sh_view_opacities", lambda: ops.sh_view_opacities(3, means, centre, dc, rest)
    P, L = N, 3
    seg = (torch.arange(L * P + 1, dtype=torch.int64) * 2).to(DEV)
    sel = (seg, R(3), torch.eye(3, device=DEV), R(P, 2), R(P, 2) + 1, torch.tensor([1.0, 2.0], device=DEV),
           torch.zeros(P, dtype=torch.int8, device=DEV), torch.ones(P, dtype=torch.uint8, device=DEV))
    yield "lod_select", lambda: ops.lod_select(*sel)
    pm = (R(N, 3), R(N, 3), R(N, 1), R(N, 1) + 0.5, R(N, 1))
    yield "pvg_motion", lambda: ops.pvg_motion(*pm, 0.3, 1.0)
    levels = ops.hashgrid_levels(3, 4, 2, 12, 4, 1.5)
    x, table = R(N, 3), ops.hashgrid_table(levels, device=DEV)
    yield "hashgrid_encode", lambda: ops.hashgrid_encode(x, table, levels)
    layout = ops.hexplane_layout([8, 8, 8, 4], [1, 2], 8)
    htable, box = R(layout.total, 8), ops.hexplane_box(np.array([[1.0] * 3, [-1.0] * 3], np.float32))
    yield "hexplane_encode", lambda: ops.hexplane_encode(x, 0.5, htable, box, layout)


result = {"label": label, "n": N, "calls": 2000, "warmup": 200, "median_us": {}}
for name, call in cases():
    for _ in range(200):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(2000):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    result["median_us"][name] = round(statistics.median(times) * 1e6, 3)
print(json.dumps(result), flush=True)
