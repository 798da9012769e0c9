"""LPIPS-VGG on the device: the perceptual distance the reference trains with (`lpips.LPIPS(net="vgg")`,
xparam/modules/denoising_diffusion.py:47,331-336), whose weights its checkpoints carry under `loss_fn_vgg.` (include/cdc_hip.h:
cdc_lpips states the definition; kernels in csrc/lpips_kernels.hip, the network program in csrc/cdc_planner.hip).

`LpipsVGG` mirrors the module as the other classes of this package mirror theirs: `load_state_dict` takes the names of lpips 0.1.4
below a prefix, `model(a, b)` returns the distance per image as float64.  The state-dict names are written from that package's source
as remembered (it is not installed here); the library's manifest is the one place that holds them.  This is the metric, not the
training loss: there are no gradients."""
import numpy as np

from . import _lib
from .unet import _as_host_f32

PREFIX = "loss_fn_vgg."       # where GaussianDiffusion.state_dict() of the reference keeps the network
# accepted beside the manifest: the copies the package's ModuleList registers (they must equal lin{k}) and the scaling layer's buffers
OPTIONAL = tuple(f"lins.{k}.model.1.weight" for k in range(5)) + ("scaling_layer.shift", "scaling_layer.scale")
MIN_SIDE = 16


class LpipsVGG:
    def __init__(self, device=None):
        self.training = False
        self._lh = _lib.Handle("cdc_lpips_create", None, _lib.device_index_of(device))

    # ---- handle management (_lib.Handle): created on first use; the parameters become final (on the GPU) with the first computation
    def _handle(self):
        return self._lh.ptr

    _h = property(lambda self: self._lh.raw)
    _finalized = property(lambda self: self._lh.finalized)
    device_index = property(lambda self: self._lh.device_index)

    def _ready(self):
        """The handle with final weights (what a computation needs: this is where a host without a GPU fails)."""
        h = self._handle()
        if not self._finalized:
            if not self._lh.tensors:
                raise _lib.CdcError("load_state_dict() has not been called")
            self._lh.finalize()
        return h

    def status(self):
        return self._lh.status()

    def to(self, device):
        self._lh.move(_lib.device_index_of(device))
        return self

    def eval(self):
        self.training = False
        return self

    # ---- parameters
    def manifest(self):
        """[(name, shape)] of the required entries, below the prefix."""
        return self._lh.manifest()

    def load_state_dict(self, state_dict, prefix=None, strict=True):
        """The entries below `prefix`; None: "loss_fn_vgg." when keys carry it (a whole reference checkpoint), else none.
        strict: every required entry must be there and nothing else below the prefix.  A `lins.{k}` copy must equal `lin{k}`."""
        if prefix is None:
            prefix = PREFIX if any(k.startswith(PREFIX) for k in state_dict) else ""
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        man = self.manifest()
        names = [n for n, _ in man]
        missing = [n for n in names if n not in sd]
        unexpected = [k for k in sd if k not in names and k not in OPTIONAL]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for LpipsVGG: missing {missing[:3]}{'...' if len(missing) > 3 else ''}, "
                               f"unexpected {unexpected[:3]}")
        for n, shape in man:
            if n in sd and tuple(sd[n].shape) != tuple(shape):
                raise RuntimeError(f"size mismatch for {n}: got {tuple(sd[n].shape)}, expected {tuple(shape)}")
        for k in range(5):
            lin, dup = f"lin{k}.model.1.weight", f"lins.{k}.model.1.weight"
            if dup in sd and lin in sd and not np.array_equal(_as_host_f32(sd[dup]), _as_host_f32(sd[lin])):
                raise RuntimeError(f"{prefix}{dup} differs from {prefix}{lin}: the two names hold one parameter")
        for n in names + list(OPTIONAL):
            if n in sd:
                self._lh.load(n, _as_host_f32(sd[n]))
        return self

    def state_dict(self):
        return dict(self._lh.tensors)

    # ---- the distance
    def forward(self, a, b, size=None, as_saved=False, return_layers=False):
        """LPIPS per image over the top-left `size=(H, W)` window (default: the operands' common shape), float64 [B]; operands and
        `as_saved` as for metrics.psnr.  return_layers: also the five layer values [B, 5] whose sum it is."""
        from . import metrics
        return metrics.lpips(self, a, b, size=size, as_saved=as_saved, return_layers=return_layers)

    __call__ = forward
