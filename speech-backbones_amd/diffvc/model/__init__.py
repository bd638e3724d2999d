"""DiffVC's `model` package: `from model import DiffVC` (DiffVC/inference.ipynb), `from model.diffusion import Diffusion`,
`from model.utils import FastGL, sequence_mask` (DiffVC/train_dec.py, train_enc.py).

With `speech-backbones_amd/diffvc` on sys.path this file is found as the top-level package `model`, as DiffVC's scripts import it.  Its
modules share code with the Grad-TTS package beside it through package-relative imports, so the top-level name is made an alias of the
package under its full name: `model`, `model.utils`, ... are then the very module objects of `<package>.diffvc.model`."""
if "." in __name__:
    from .diffusion import Diffusion, GradLogPEstimator  # noqa: F401
    from .vc import DiffVC, FwdDiffusion  # noqa: F401
else:
    import importlib
    import os
    import sys

    _pkg_dir = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if os.path.dirname(_pkg_dir) not in sys.path:
        sys.path.append(os.path.dirname(_pkg_dir))
    _real = importlib.import_module(os.path.basename(_pkg_dir) + ".diffvc.model")
    for _name, _mod in list(sys.modules.items()):
        if _name.startswith(_real.__name__ + "."):
            sys.modules[__name__ + _name[len(_real.__name__):]] = _mod
    sys.modules[__name__] = _real
