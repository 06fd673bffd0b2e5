"""The reference's UNCHANGED LightningModule trains on the 3DGS-MCMC route of this repository: `HipMCMCDensityController`,
`HipMCMCMetrics` and `HipVanillaRenderer` selected as `--model.density / --model.metric / --model.renderer` would select them, with the
reference's own `VanillaGaussian` model, `Cameras`, optimizers and schedulers (tests/mcmc_loop_worker.py, in a process of its own under
tests/lightning_standin.py).  No GPU here and no reference tree on the GPU box: the native ops under the plugins are the fp64 oracles
(their HIP parity is what tests/test_mcmc_gpu.py establishes).

Checked over 300 steps, on the model's raw parameters and on its activated getters: relocation events fire where the configuration
says; each event grows the count to min(cap_max, int(1.05 n)) until cap_max; every Gaussian at or below min_opacity is relocated by the
event (none survives untouched); the noise hook — appended by `setup("fit")` to the module's `on_train_batch_end_hooks` — ran after
every step, the last one included (the reference's final-step guard never fires); the regulariser of `HipMCMCMetrics` ran every step;
the loss falls."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = os.environ.get("GSPL_REFERENCE_ROOT", "/root/reference")
needs_reference = pytest.mark.skipif(not os.path.exists(os.path.join(REF_ROOT, "internal", "gaussian_splatting.py")),
                                     reason="reference tree not present")
STEPS = 300


def _run(variant):
    r = subprocess.run([sys.executable, os.path.join(HERE, "mcmc_loop_worker.py"), REF_ROOT, str(STEPS), variant],
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@needs_reference
@pytest.mark.parametrize("variant", ["raw", "activated"])
def test_unchanged_lightning_module_trains_on_the_mcmc_plugins(variant):
    d = _run(variant)
    assert d["controller"] == "gspl_amd.mcmc.HipMCMCDensityControllerImpl" and d["metric"] == "gspl_amd.mcmc.HipMCMCMetricsImpl"
    assert d["hooks"] == 1 and d["init_opacity"] == pytest.approx(0.5)
    losses, counts = d["losses"], d["counts"]
    assert len(losses) == STEPS and all(np.isfinite(losses))

    # the hook ran after every step, the regulariser in every step, on the path the variant selects
    assert d["noise_calls"] == list(range(1, STEPS + 1)) and d["reg_calls"] == list(range(1, STEPS + 1))
    raw = STEPS if variant == "raw" else 0
    assert d["calls"]["noise_raw"] == raw and d["calls"]["reg_raw"] == raw
    assert all(np.isfinite(d["o_regs"])) and d["o_regs"][0] == pytest.approx(0.01 * 0.5, rel=1e-5)

    # events where the configuration puts them: global steps in (from, until), multiples of the interval
    f, iv, until = d["densify"]["from"], d["densify"]["interval"], d["densify"]["until"]
    expected_steps = [s for s in range(1, STEPS + 1) if f < s < until and s % iv == 0]
    events = d["events"]
    assert len(events) == len(expected_steps) > 0
    assert sum(e["dead"] for e in events) > 0, "no relocation of dead Gaussians happened"
    for e in events:
        assert e["n_after"] == min(d["cap_max"], int(1.05 * e["n_before"])), e
        assert e["dead_rows_replaced"] and e["low_opacity_untouched"] == 0, e
    assert events[0]["n_before"] == d["n0"] and counts[-1] == d["cap_max"]
    grew = [e for e in events if e["added"] > 0]
    assert len(grew) >= 3 and events[-1]["added"] == 0
    # the count only changes at events
    changes = [i + 1 for i in range(1, STEPS) if counts[i] != counts[i - 1]]
    assert set(changes) <= set(expected_steps)

    assert np.mean(losses[-30:]) < 0.5 * np.mean(losses[:30]), (losses[:5], losses[-5:])
