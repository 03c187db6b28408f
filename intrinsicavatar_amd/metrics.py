"""Frame evaluation on the device (csrc/metrics.hip): what the reference computes between "the model returned its maps" and "a number
is logged" -- systems/criterions.py:43-102, models/utils.py:268-277, systems/intrinsic_avatar.py:303-315 and :380-399.

    PSNR()(inputs, targets, valid_mask=None)                 -10 log10(mean((inputs - targets)^2 [valid_mask]))        0-d float32
    SSIM()(inputs, targets, valid_mask=None)                 scikit-image 0.18.1's structural_similarity(multichannel=True) of two
                                                             [H,W,C] images, cropped to the mask's bounding rectangle  0-d float64
    NormalError()(inputs, targets, valid_mask)               mean angle in degrees over the mask                       0-d float32
    compute_albedo_rescale_factor(gt, pred, mask)            per channel sum(gt pred) / sum(pred pred) over the mask   [3] float32
    align_albedo(gt, pred, mask, ratio=None)                 mask ? clamp(ratio pred, 0, 1) : 0                        [n,3] float32
    transform_normals(normals, w2c=None)                     world -> OpenGL camera space                              [n,3] float32
    mask_rect(mask)                                          cv2.boundingRect of an [H,W] mask                         [4] int32
    LPIPSNet.from_state_dicts(vgg16, lin, device)            lpips.LPIPS(net="vgg") from the torchvision vgg16 and lpips v0.1 state dicts
    net(in0, in1, normalize=False, rect=None)                the package's forward on [N,3,H,W] pairs (csrc/lpips.hip)  [N,1,1,1] float32
    LPIPS()(inputs, targets, loss_fn_vgg, valid_mask=None)   that distance of two [H,W,3] images in [0,1], cropped to
                                                             the mask's bounding rectangle on the device               0-d float32

Inputs are GPU tensors (CPU tensors raise: there is no host route); results are DEVICE tensors and nothing is read back until the
caller converts one.  A value that cannot be formed -- an empty mask, a rectangle with a side shorter than the 7-pixel window (16
pixels for LPIPS: five taps, four poolings) -- is NaN on the device and carries a status word next to it: `.item()`, `float()`,
`.tolist()` and `.cpu()` of the returned MetricValue read value and status in ONE copy and raise ValueError then; to_host() does so
for a whole dict of metrics with one copy in all.  Every reduction is deterministic (DESIGN.md "Frame evaluation").

LPIPS: the key names of the two state dicts, the five tap positions and the constants of the scaling layer are taken from the published
layout of torchvision and lpips; neither package was at hand, so no run against their weights has been made."""
from typing import Dict, List, Optional, Sequence

import torch
from torch import Tensor

from . import _lib as L

_STATUS = {1: "nothing to average: the mask is empty, or a side of the rectangle is shorter than the 7-pixel SSIM window",
           2: "the rectangle does not lie inside the image",
           3: "nothing is left at the fifth LPIPS tap: the mask is empty, or a side of the rectangle is shorter than 16 pixels"}


class MetricValue(Tensor):
    """a device tensor that is a view of `_buf` = (value..., status): converting it to a host number checks the status."""

    @staticmethod
    def make(buf: Tensor, n_values: int, what: str) -> "MetricValue":
        v = (buf[0] if n_values == 1 else buf[:n_values]).as_subclass(MetricValue)
        v._buf, v._what = buf, what
        return v

    def checked(self) -> Tensor:
        """the value on the HOST (plain tensor) after one copy of (value, status); ValueError if it could not be formed."""
        buf = getattr(self, "_buf", None)
        if buf is None:                                  # a tensor derived from a metric: an ordinary tensor
            return self.as_subclass(Tensor).cpu()
        host = buf.as_subclass(Tensor).cpu()
        _raise_on_status(int(host[-1]), self._what)
        return host[0] if self.dim() == 0 else host[:-1].reshape(self.shape)

    def item(self):
        return self.checked().item()

    def tolist(self):
        return self.checked().tolist()

    def cpu(self, *a, **k):
        return self.checked()

    def __float__(self):
        return float(self.checked())


def _raise_on_status(status: int, what: str):
    if status != 0:
        raise ValueError(f"{what}: {_STATUS.get(status, f'status {status}')}")


def to_host(metrics: Dict[str, Tensor]) -> Dict[str, float]:
    """every metric of a dict as a Python float (lists for vectors) with ONE device-to-host copy; ValueError on a bad status."""
    bufs = {k: getattr(v, "_buf", None) for k, v in metrics.items()}
    parts = [(b if b is not None else metrics[k].reshape(-1)).as_subclass(Tensor).double().reshape(-1) for k, b in bufs.items()]
    host = torch.cat(parts).cpu() if parts else torch.zeros(0)
    out, o = {}, 0
    for (k, b), p in zip(bufs.items(), parts):
        vals = host[o:o + p.numel()]
        o += p.numel()
        if b is not None:
            _raise_on_status(int(vals[-1]), k)
            vals = vals[:-1]
        out[k] = float(vals[0]) if metrics[k].dim() == 0 else vals.tolist()
    return out


def _f32(t: Tensor, what: str) -> Tensor:
    if not isinstance(t, Tensor) or not t.is_cuda:
        raise L.IaError(f"{what}: intrinsicavatar_amd.metrics needs GPU tensors (no CPU fallback)")
    return t.detach().as_subclass(Tensor).float().contiguous()


def _mask(m: Optional[Tensor], n: int, what: str) -> Optional[Tensor]:
    if m is None:
        return None
    if not m.is_cuda:
        raise L.IaError(f"{what}: intrinsicavatar_amd.metrics needs GPU tensors (no CPU fallback)")
    if m.numel() != n:
        raise ValueError(f"{what}: the mask has {m.numel()} entries for {n} rows")
    m = m.detach().reshape(-1)
    return (m if m.dtype == torch.bool else m != 0).contiguous().view(torch.uint8)


def _tmp(dev) -> Tensor:
    return L.work_area(L.lib().ia_metric_tmp_bytes(), dev)


def squared_error(inputs: Tensor, targets: Tensor, valid_mask: Optional[Tensor] = None):
    """-> (sums [2] float64 on the device = (sum of squared differences, number of elements), psnr MetricValue).  valid_mask selects
    along the leading dimensions it covers, as `value[valid_mask]` does."""
    a, b = _f32(inputs, "PSNR"), _f32(targets, "PSNR")
    if a.shape != b.shape:
        raise ValueError(f"PSNR: shapes differ: {tuple(a.shape)} and {tuple(b.shape)}")
    if valid_mask is not None:
        n = valid_mask.numel()
        if n == 0 or a.numel() % n or tuple(a.shape[:valid_mask.dim()]) != tuple(valid_mask.shape):
            raise ValueError(f"PSNR: a mask of shape {tuple(valid_mask.shape)} does not index maps of shape {tuple(a.shape)}")
        c = a.numel() // n
    else:
        n, c = a.numel(), 1
    dev = a.device
    sums = torch.empty(2, dtype=torch.float64, device=dev)
    buf = torch.empty(2, dtype=torch.float32, device=dev)
    L.lib().ia_metric_sq_err(n, c, a, b, _mask(valid_mask, n, "PSNR"), _tmp(dev), sums, buf)
    return sums, MetricValue.make(buf, 1, "PSNR")


class PSNR(torch.nn.Module):
    def forward(self, inputs, targets, valid_mask=None, reduction="mean"):
        assert reduction in ["mean", "none"]
        if reduction == "none":
            raise NotImplementedError("PSNR(reduction='none') is not provided: no call site of the reference uses it")
        return squared_error(inputs, targets, valid_mask)[1]


def normal_error(inputs: Tensor, targets: Tensor, valid_mask: Optional[Tensor], *, w2c: Optional[Tensor] = None, transform: bool = False,
                 normalize: bool = False, want_map: bool = False, want_camera: bool = False):
    """NormalError.forward with the steps in front of it fused on request: transform (transform_normals of `inputs`, with w2c when
    given), normalize (F.normalize on both sides).  -> dict(mean=MetricValue, sums=[2] float64 (sum error, sum mask),
    map=[...] float32 per-pixel degrees x mask (want_map), camera=[n,3] the transformed, un-normalised inputs (want_camera))."""
    a, b = _f32(inputs, "NormalError"), _f32(targets, "NormalError")
    if a.shape != b.shape or a.shape[-1] != 3:
        raise ValueError(f"NormalError: needs two [..., 3] maps of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    n, dev = a.numel() // 3, a.device
    rot = _rotation(w2c) if transform else None
    sums = torch.empty(2, dtype=torch.float64, device=dev)
    buf = torch.empty(2, dtype=torch.float32, device=dev)
    err = torch.empty(a.shape[:-1], dtype=torch.float32, device=dev) if want_map else None
    cam = torch.empty_like(a) if (want_camera and transform) else None
    L.lib().ia_metric_normal_error(n, a, b, _mask(valid_mask, n, "NormalError"), rot, int(transform), int(normalize), cam, err, _tmp(dev), sums, buf)
    return dict(mean=MetricValue.make(buf, 1, "NormalError"), sums=sums, map=err, camera=cam)


class NormalError(torch.nn.Module):
    def forward(self, inputs, targets, valid_mask, reduction="mean"):
        assert reduction in ["mean", "none"]
        r = normal_error(inputs, targets, valid_mask, want_map=reduction == "none")
        return r["mean"] if reduction == "mean" else r["map"]


def _rotation(w2c: Optional[Tensor]) -> Optional[Tensor]:
    """the [3,3] block transform_normals multiplies by, from a [1,4,4] / [4,4] / [3,3] world-to-camera matrix."""
    if w2c is None:
        return None
    if not w2c.is_cuda:
        raise L.IaError("transform_normals: intrinsicavatar_amd.metrics needs GPU tensors (no CPU fallback)")
    if w2c.dim() == 3:
        assert w2c.shape[0] == 1 and w2c.shape[1] == 4 and w2c.shape[2] == 4
        w2c = w2c[0]
    return w2c[:3, :3].detach().float().contiguous()


def transform_normals(normals: Tensor, w2c: Optional[Tensor] = None) -> Tensor:
    """world-space normal map -> OpenGL camera space: normals @ w2c[:3,:3]^T when w2c is given, then x (1, -1, -1)."""
    a = _f32(normals, "transform_normals")
    if a.shape[-1] != 3:
        raise ValueError(f"transform_normals: needs a [..., 3] map, got {tuple(a.shape)}")
    out = torch.empty_like(a)
    L.lib().ia_metric_transform_normals(a.numel() // 3, a, _rotation(w2c), out)
    return out


def albedo_sums(gt_albedo: Tensor, pred_albedo: Tensor, gt_mask: Optional[Tensor]):
    """-> (sums [3,2] float64 on the device = per channel (sum gt pred, sum pred pred) over the mask, ratio MetricValue [3] float32)."""
    x, xh = _f32(gt_albedo, "compute_albedo_rescale_factor"), _f32(pred_albedo, "compute_albedo_rescale_factor")
    if x.shape != xh.shape or x.shape[-1] != 3:
        raise ValueError(f"compute_albedo_rescale_factor: needs two [..., 3] maps of one shape, got {tuple(x.shape)} and {tuple(xh.shape)}")
    n, dev = x.numel() // 3, x.device
    sums = torch.empty((3, 2), dtype=torch.float64, device=dev)
    buf = torch.empty(4, dtype=torch.float32, device=dev)
    L.lib().ia_metric_albedo_sums(n, x, xh, _mask(gt_mask, n, "compute_albedo_rescale_factor"), _tmp(dev), sums, buf)
    return sums, MetricValue.make(buf, 3, "compute_albedo_rescale_factor")


def compute_albedo_rescale_factor(gt_albedo: Tensor, pred_albedo: Tensor, gt_mask: Tensor) -> Tensor:
    return albedo_sums(gt_albedo, pred_albedo, gt_mask)[1]


def align_albedo(gt_albedo: Tensor, pred_albedo: Tensor, gt_mask: Tensor, ratio: Optional[Tensor] = None):
    """the reference's three_aligned_albedo: zeros_like(gt), and on the mask clamp(ratio * pred, 0, 1); the ratio is computed from
    (gt, pred, mask) when it is not given.  -> (aligned [n,3] float32, ratio [3])."""
    if ratio is None:
        ratio = compute_albedo_rescale_factor(gt_albedo, pred_albedo, gt_mask)
    xh = _f32(pred_albedo, "align_albedo")
    n = xh.numel() // 3
    out = torch.empty_like(xh)
    L.lib().ia_metric_albedo_apply(n, xh, _mask(gt_mask, n, "align_albedo"), _f32(ratio, "align_albedo"), out)
    return out, ratio


def mask_rect(mask: Tensor) -> Tensor:
    """(x, y, w, h) int32 on the device of the non-zero pixels of an [H,W] mask -- cv2.boundingRect; (0, 0, 0, 0) when there is none."""
    if mask.dim() != 2:
        raise ValueError(f"mask_rect: needs an [H, W] mask, got {tuple(mask.shape)}")
    H, W = (int(s) for s in mask.shape)
    m = _mask(mask, H * W, "mask_rect")
    rect = torch.empty(4, dtype=torch.int32, device=mask.device)
    L.lib().ia_metric_mask_rect(H, W, m, _tmp(mask.device), rect)
    return rect


def ssim(inputs: Tensor, targets: Tensor, rect: Optional[Tensor] = None) -> MetricValue:
    """mean SSIM of two [H,W,C] images over rect = (x, y, w, h) int32 ON THE DEVICE (None: the whole image); 0-d float64."""
    a, b = _f32(inputs, "SSIM"), _f32(targets, "SSIM")
    if a.shape != b.shape or a.dim() != 3:
        raise ValueError(f"SSIM: needs two [H, W, C] images of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    H, W, Cn = (int(s) for s in a.shape)
    if rect is not None:
        if not rect.is_cuda or rect.dtype != torch.int32 or rect.numel() != 4:
            raise ValueError("SSIM: rect must be 4 int32 values on the device (mask_rect's output)")
        rect = rect.contiguous()
    dev = a.device
    tmp = L.work_area(L.lib().ia_metric_ssim_tmp_bytes(H, W, Cn), dev)
    buf = torch.empty(2, dtype=torch.float64, device=dev)
    L.lib().ia_metric_ssim(H, W, Cn, a, b, rect, tmp, buf)
    return MetricValue.make(buf, 1, "SSIM")


class SSIM(torch.nn.Module):
    def forward(self, inputs, targets, valid_mask=None):
        rect = None
        if valid_mask is not None:
            assert valid_mask.dtype == torch.bool
            rect = mask_rect(valid_mask)
        return ssim(inputs, targets, rect)


# ------------------------------------------------------------------------- LPIPS (csrc/lpips.hip)
# (torchvision `features` index, Cin, Cout) of the 13 convolutions of vgg16; a 2 x 2 max-pool sits in front of VGG_POOL_BEFORE, and the
# ReLU outputs after VGG_TAPS are the five feature maps lpips compares (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3)
VGG_CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (17, 256, 512),
             (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512))
VGG_POOL_BEFORE = (5, 10, 17, 24)
VGG_TAPS = (2, 7, 14, 21, 28)
LPIPS_MIN_SIDE = 1 << (len(VGG_TAPS) - 1)


def _rect(rect: Optional[Tensor], what: str) -> Optional[Tensor]:
    if rect is None:
        return None
    if not rect.is_cuda or rect.dtype != torch.int32 or rect.numel() != 4:
        raise ValueError(f"{what}: rect must be 4 int32 values on the device (mask_rect's output)")
    return rect.contiguous()


def pack_conv3x3(weight: Tensor, bias: Tensor, device):
    """a torch convolution's weight [Cout,Cin,3,3] and bias [Cout] -> (wpk [9, Cin rounded up to 4, Cout], bias) float32 on `device`:
    tap-major, output channel innermost (the layout ia_lpips_conv3x3 stages); the added input channels are zero."""
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    w = weight.detach().to(device=device, dtype=torch.float32).permute(2, 3, 1, 0).reshape(9, cin, cout)
    pad = -cin % 4
    if pad:
        w = torch.cat([w, torch.zeros((9, pad, cout), dtype=torch.float32, device=device)], dim=1)
    return w.contiguous(), bias.detach().to(device=device, dtype=torch.float32).contiguous()


def lpips_input(img: Tensor, normalize: bool = False, rect: Optional[Tensor] = None) -> Tensor:
    """[N,H,W,3] in [0,1] -> [N,H,W,4]: the rectangle moved to the origin, 2x - 1 on request, the scaling layer; channel 3 is zero.
    Only [:, :h, :w] of the result is defined when a rectangle is given."""
    x = _f32(img, "LPIPS")
    if x.dim() != 4 or x.shape[-1] != 3:
        raise ValueError(f"LPIPS: needs [N, H, W, 3] images, got {tuple(x.shape)}")
    N, H, W = (int(s) for s in x.shape[:3])
    out = torch.empty((N, H, W, 4), dtype=torch.float32, device=x.device)
    L.lib().ia_lpips_input(N, H, W, x, _rect(rect, "LPIPS"), int(bool(normalize)), out)
    return out


def lpips_conv3x3(x: Tensor, wpk: Tensor, bias: Tensor, rect: Optional[Tensor] = None, level: int = 0, at_rect: bool = False) -> Tensor:
    """relu(conv3x3(x [N,H,W,Cin], pad 1) + bias) -> [N,H,W,Cout] with pack_conv3x3's operands.  With a rectangle the layer runs over
    its extent (h >> level, w >> level) -- read at the rectangle's corner when at_rect, else at the origin -- and writes [:, :h, :w]."""
    x = _f32(x, "LPIPS")
    N, H, W, cin = (int(s) for s in x.shape)
    if int(wpk.shape[1]) != cin:
        raise ValueError(f"LPIPS: the layer takes {int(wpk.shape[1])} channels, the input has {cin}")
    out = torch.empty((N, H, W, int(wpk.shape[2])), dtype=torch.float32, device=x.device)
    L.lib().ia_lpips_conv3x3(N, H, W, cin, int(wpk.shape[2]), x, wpk, bias, out, _rect(rect, "LPIPS"), int(level), int(bool(at_rect)))
    return out


def lpips_maxpool2(x: Tensor, rect: Optional[Tensor] = None, level: int = 0) -> Tensor:
    """max_pool2d(kernel 2) of [N,H,W,C] -> [N,H//2,W//2,C]; x is a buffer of `level` when a rectangle is given."""
    x = _f32(x, "LPIPS")
    N, H, W, C = (int(s) for s in x.shape)
    out = torch.empty((N, H >> 1, W >> 1, C), dtype=torch.float32, device=x.device)
    L.lib().ia_lpips_maxpool2(N, H, W, C, x, out, _rect(rect, "LPIPS"), int(level))
    return out


class LPIPSNet(torch.nn.Module):
    """lpips.LPIPS(net="vgg") (version 0.1, the linear layers on): forward(in0, in1, normalize=False, rect=None) on [N,3,H,W] pairs ->
    [N,1,1,1] float32 on the device.  features() / distance() are its two halves on NHWC images, so that an image compared with
    several others (a frame's ground truth) goes through the trunk once; an image's features do not depend on its batch slot."""

    def __init__(self, convs: Sequence, lins: Sequence[Tensor]):
        super().__init__()
        self.convs, self.lins = list(convs), list(lins)

    @staticmethod
    def check_state_dicts(vgg16_state, lin_state) -> None:
        """host only: ValueError naming the first key that is missing or has the wrong shape."""
        for idx, cin, cout in VGG_CONVS:
            for key, shape in ((f"features.{idx}.weight", (cout, cin, 3, 3)), (f"features.{idx}.bias", (cout,))):
                if key not in vgg16_state:
                    raise ValueError(f"LPIPSNet: the vgg16 state dict has no {key}")
                if tuple(vgg16_state[key].shape) != shape:
                    raise ValueError(f"LPIPSNet: {key} has shape {tuple(vgg16_state[key].shape)}, expected {shape}")
        for i, tap in enumerate(VGG_TAPS):
            key, shape = f"lin{i}.model.1.weight", (1, dict((c[0], c[2]) for c in VGG_CONVS)[tap], 1, 1)
            if key not in lin_state:
                raise ValueError(f"LPIPSNet: the lpips state dict has no {key}")
            if tuple(lin_state[key].shape) != shape:
                raise ValueError(f"LPIPSNet: {key} has shape {tuple(lin_state[key].shape)}, expected {shape}")

    @classmethod
    def from_state_dicts(cls, vgg16_state, lin_state, device) -> "LPIPSNet":
        """torchvision's vgg16 state dict (features.{0,2,...,28}.{weight,bias}) + the lpips v0.1 state dict (lin{0..4}.model.1.weight):
        the weights are packed for the kernels here, once."""
        cls.check_state_dicts(vgg16_state, lin_state)
        if torch.device(device).type != "cuda":
            raise L.IaError("LPIPSNet: intrinsicavatar_amd.metrics needs a GPU device (no CPU fallback)")
        convs = [pack_conv3x3(vgg16_state[f"features.{idx}.weight"], vgg16_state[f"features.{idx}.bias"], device) for idx, _, _ in VGG_CONVS]
        lins = [lin_state[f"lin{i}.model.1.weight"].detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous()
                for i in range(len(VGG_TAPS))]
        return cls(convs, lins)

    @classmethod
    def from_files(cls, vgg_path: str, lin_path: str, device) -> "LPIPSNet":
        return cls.from_state_dicts(torch.load(vgg_path, map_location="cpu", weights_only=True),
                                    torch.load(lin_path, map_location="cpu", weights_only=True), device)

    def features(self, img: Tensor, normalize: bool = False, rect: Optional[Tensor] = None) -> List[Tensor]:
        """img [N,H,W,3] in [0,1] ([-1,1] without normalize) -> the five taps, [N, H >> l, W >> l, C_l]; with a rectangle (x, y, w, h)
        on the device, [:, :h >> l, :w >> l] of each holds the features of the crop and the rest is undefined."""
        rect = _rect(rect, "LPIPS")
        cur = lpips_input(img, normalize, rect)
        N, h, w = (int(s) for s in cur.shape[:3])
        if min(h, w) < LPIPS_MIN_SIDE:
            raise ValueError(f"LPIPS: needs images of at least {LPIPS_MIN_SIDE} x {LPIPS_MIN_SIDE} pixels, got {h} x {w}")
        level, taps = 0, []
        for (idx, _, _), (wpk, bias) in zip(VGG_CONVS, self.convs):
            if idx in VGG_POOL_BEFORE:
                cur = lpips_maxpool2(cur, rect, level)
                level += 1
            cur = lpips_conv3x3(cur, wpk, bias, rect, level)
            if idx in VGG_TAPS:
                taps.append(cur)
        return taps

    def distance(self, f0: Sequence[Tensor], f1: Sequence[Tensor], rect: Optional[Tensor] = None) -> Tensor:
        """two results of features() with the same rectangle -> [N + 1] float32 on the device: the N distances, then the status."""
        rect = _rect(rect, "LPIPS")
        N, H, W = (int(s) for s in f0[0].shape[:3])
        if len(f0) != len(self.lins) or len(f1) != len(self.lins) or any(
                a.shape != b.shape or tuple(a.shape) != (N, H >> l, W >> l, lin.numel()) for l, (a, b, lin) in enumerate(zip(f0, f1, self.lins))):
            raise ValueError("LPIPS: the two feature lists are not features() of two batches of one shape")
        dev = f0[0].device
        cap = -(-H * W // int(L.lib().ia_lpips_pixels_per_partial()))
        partials = torch.empty((len(self.lins), N, cap), dtype=torch.float64, device=dev)
        for l, (a, b, lin) in enumerate(zip(f0, f1, self.lins)):
            L.lib().ia_lpips_layer_dist(N, H >> l, W >> l, int(a.shape[-1]), a, b, lin, rect, l, partials[l], cap)
        buf = torch.empty(N + 1, dtype=torch.float32, device=dev)
        L.lib().ia_lpips_finish(N, H, W, rect, partials, cap, buf)
        return buf

    def forward(self, in0: Tensor, in1: Tensor, normalize: bool = False, rect: Optional[Tensor] = None) -> MetricValue:
        a, b = _f32(in0, "LPIPS"), _f32(in1, "LPIPS")
        if a.shape != b.shape or a.dim() != 4 or a.shape[1] != 3:
            raise ValueError(f"LPIPS: needs two [N, 3, H, W] batches of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
        nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()      # noqa: E731
        buf = self.distance(self.features(nhwc(a), normalize, rect), self.features(nhwc(b), normalize, rect), rect)
        N = int(a.shape[0])
        v = buf[:N].reshape(N, 1, 1, 1).as_subclass(MetricValue)
        v._buf, v._what = buf, "LPIPS"
        return v


def lpips_features(loss_fn_vgg: LPIPSNet, image, rect: Optional[Tensor] = None) -> List[Tensor]:
    """the features the criterion forms of one [H,W,3] image in [0,1] (normalize=True), over the rectangle when one is given.  A
    sequence of images of one shape goes through the trunk as one batch -- slot i of the result holds the bits of a call on image i
    alone, and the deep layers of a small crop fill more of the device."""
    images = [image] if isinstance(image, Tensor) else list(image)
    xs = [_f32(t, "LPIPS") for t in images]
    if any(x.dim() != 3 or x.shape[-1] != 3 or x.shape != xs[0].shape for x in xs):
        raise ValueError(f"LPIPS: needs [H, W, 3] images of one shape, got {[tuple(x.shape) for x in xs]}")
    return loss_fn_vgg.features(xs[0][None] if len(xs) == 1 else torch.stack(xs), True, rect)


def lpips_of_features(loss_fn_vgg: LPIPSNet, f0: Sequence[Tensor], f1: Sequence[Tensor], rect: Optional[Tensor] = None,
                      slots=(0, 0)) -> MetricValue:
    """the criterion's value from image slots[0] of the features f0 and image slots[1] of f1 (lpips_features with the same rectangle)"""
    i, j = slots
    return MetricValue.make(loss_fn_vgg.distance([t[i:i + 1] for t in f0], [t[j:j + 1] for t in f1], rect), 1, "LPIPS")


class LPIPS(torch.nn.Module):
    def forward(self, inputs, targets, loss_fn_vgg, valid_mask=None):
        assert inputs.shape == targets.shape
        assert len(inputs.shape) == 3
        rect = None
        if valid_mask is not None:
            assert valid_mask.dtype == torch.bool
            rect = mask_rect(valid_mask)
        return lpips_of_features(loss_fn_vgg, lpips_features(loss_fn_vgg, inputs, rect), lpips_features(loss_fn_vgg, targets, rect), rect)
