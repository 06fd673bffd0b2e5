"""`python -m gspl_amd.launch <script> [args...]` — run one of the reference's entry points (main.py, viewer.py, utils/*.py) on a
machine that has no `diff_gaussian_rasterization` / `gsplat` / `simple_knn` / `fused_ssim` (they are CUDA packages).

The reference imports `diff_gaussian_rasterization` while `internal.renderers` is imported (internal/renderers/vanilla_renderer.py:14),
i.e. before its CLI has parsed `--model.renderer`: the stand-ins of `gspl_amd.compat` therefore have to be registered BEFORE the
entry point is imported.  This launcher does exactly that and then runs the script unchanged, as `python <script> [args...]` would:

    python -m gspl_amd.launch main.py fit --data.path data/lego --model.renderer gspl_amd.renderers.HipVanillaRenderer

It also lets `torch.optim.lr_scheduler.LambdaLR` take the `verbose=` keyword that newer torch releases removed: the reference passes
`verbose=False` (internal/output_processors/bilagrid.py and exposure.py, the appearance-embedding, deformable, SWAG and RGB-MLP
renderers).  Only in this launched process, and only when the installed torch rejects the keyword; importing the package patches
nothing in torch.

With `GSPL_HIP_GS4D=1` in the environment the viewer's `--vanilla_gs4d` route is served by the HIP plugin: the launcher binds
`internal.renderers.vanilla_gs4d_renderer.VanillaGS4DRenderer` (which internal/viewer/viewer.py imports when it builds that renderer)
to `gspl_amd.renderers.HipVanillaGS4DRenderer`, in this launched process only.  Without the variable nothing is bound.
"""
import inspect
import os
import runpy
import sys


def _lambdalr_takes_verbose(cls) -> bool:
    try:
        params = inspect.signature(cls.__init__).parameters.values()
    except (TypeError, ValueError):
        return True
    return any(p.name == "verbose" or p.kind is p.VAR_KEYWORD for p in params)


def accept_lambdalr_verbose() -> bool:
    """Replace `torch.optim.lr_scheduler.LambdaLR` by a subclass that accepts and ignores `verbose` when the installed torch rejects
    it; returns whether it did."""
    from torch.optim import lr_scheduler
    base = lr_scheduler.LambdaLR
    if _lambdalr_takes_verbose(base):
        return False

    class LambdaLR(base):
        __doc__ = base.__doc__

        def __init__(self, optimizer, lr_lambda, last_epoch=-1, verbose=None):
            super().__init__(optimizer, lr_lambda, last_epoch)

    LambdaLR.__module__, LambdaLR.__qualname__ = base.__module__, base.__qualname__
    lr_scheduler.LambdaLR = LambdaLR
    return True


def bind_gs4d_renderer() -> bool:
    """With GSPL_HIP_GS4D=1: `internal.renderers.vanilla_gs4d_renderer.VanillaGS4DRenderer` becomes the HIP plugin (same constructor,
    same model directory); returns whether it did.  The script's directory must be on sys.path already."""
    if os.environ.get("GSPL_HIP_GS4D", "0") != "1":
        return False
    import importlib
    from .renderers import HipVanillaGS4DRenderer
    importlib.import_module("internal.renderers.vanilla_gs4d_renderer").VanillaGS4DRenderer = HipVanillaGS4DRenderer
    return True


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv:
        sys.exit("usage: python -m gspl_amd.launch <script.py> [args...]")
    from . import compat
    compat.install()
    accept_lambdalr_verbose()
    script = argv[0]
    sys.argv = argv
    sys.path.insert(0, os.path.dirname(os.path.abspath(script)))      # what `python <script>` puts first
    bind_gs4d_renderer()
    runpy.run_path(script, run_name="__main__")


if __name__ == "__main__":
    main()
