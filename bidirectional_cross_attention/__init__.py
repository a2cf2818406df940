"""Drop-in for the one class GScream imports from bidirectional_cross_attention (scene/gaussian_model.py:29, built at :161-167).

The package is not part of the ROCm stack; with this directory on sys.path the reference's
`from bidirectional_cross_attention import BidirectionalCrossAttention` resolves here.  Constructor, parameter names and forward are
those of the published 0.0.4 (gscream.yaml:78); gscream_amd/crossattn.py describes them and the HIP / torch routing."""
from gscream_amd.crossattn import BidirectionalCrossAttention

__all__ = ["BidirectionalCrossAttention"]
