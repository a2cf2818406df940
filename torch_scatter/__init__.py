"""Drop-in for the one function GScream imports from torch_scatter (scene/gaussian_model.py:20, used at :874).

torch_scatter is a compiled CUDA extension that is not built for ROCm; with this directory on sys.path the reference's
`from torch_scatter import scatter_max` resolves here.  The contract is torch_scatter 2.x's documented one (see
gscream_amd/scatter.py, where ties and the HIP / torch routing are described)."""
from gscream_amd.scatter import scatter_max

__all__ = ["scatter_max"]
