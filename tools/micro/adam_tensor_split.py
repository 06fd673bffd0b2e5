"""usage (on the GPU box): GSPL_HIP_LIB=<variant .so> python tools/micro/adam_tensor_split.py
Launch time of gspl_selective_adam_rows alone at the flagship's shapes, split by tensor: N = 1 M rows, the model's six tensors (3, 3, 4, 1,
3, 45 floats per row), a given share of the rows live (chosen at random: moments non-zero), 14 % of all rows (every live one where fewer are live) flagged as
having a gradient this step.  HIP events around each of 30 launches after 5; median, min, max.  Parts: all six tensors, shs_rest alone, the five narrow
tensors alone; at 22.85 % live rows (the default bench line), 5 % and with every row live (the reference-shaped loop)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import gspl_amd  # noqa: E402,F401
from gspl_amd import _lib as L  # noqa: E402

dev = torch.device("cuda:0")
N = 1_000_000
WIDTHS = (3, 3, 4, 1, 3, 45)
g = torch.Generator().manual_seed(1)


def run(widths, live_share, label):
    live = torch.rand(N, generator=g) < live_share
    flagged = live & (torch.rand(N, generator=g) < 0.14 / max(live_share, 0.14))
    rows = flagged.to(torch.uint8).to(dev)
    items = []
    for w in widths:
        p = torch.randn(N, w, device=dev)
        m = torch.zeros(N, w, device=dev)
        v = torch.zeros(N, w, device=dev)
        m[live.to(dev)] = 0.01
        v[live.to(dev)] = 0.001
        gr = torch.zeros(N, w, device=dev)
        gr[flagged.to(dev)] = 0.01
        items.append((p, gr, m, v, 1e-4, w))
    table = (L.AdamTensor * len(items))()
    for k, (p, gr, m, v, lr, w) in enumerate(items):
        table[k] = L.AdamTensor(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), lr, w)

    def launch(step):
        L.call("gspl_selective_adam_rows", len(items), table, N, L.ptr(None), L.ptr(rows), 0.9, 0.999, 1e-15, 1 - 0.9 ** step, (1 - 0.999 ** step) ** 0.5, 0, L.stream())
    for s in range(1, 6):
        launch(s)
    torch.cuda.synchronize()
    ts = []
    for s in range(6, 36):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); launch(s); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    print(f"   {label:28s} median {ts[len(ts) // 2]:7.1f} us  min {ts[0]:7.1f}  max {ts[-1]:7.1f}", flush=True)


L.lib()
for share, what in ((0.2285, "22.85 % live"), (0.05, "5 % live"), (1.0, "all live")):
    run(WIDTHS, share, "six tensors, " + what)
    run((45,), share, "shs_rest alone, " + what)
    run(WIDTHS[:5], share, "narrow five, " + what)
