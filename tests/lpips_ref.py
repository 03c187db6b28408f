"""A plain torch restatement of lpips.LPIPS(net="vgg") (version 0.1, linear layers on) in a chosen dtype, for CPU tensors: the scaling
layer, torchvision's vgg16 `features` up to relu5_3, the five taps, unit-normalised feature differences, the 1 x 1 `lin` layers, the
spatial mean, the sum over the layers.  Shared by tests/test_lpips_cpu.py and tests/test_gpu_lpips.py."""
import torch
import torch.nn.functional as F

CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (17, 256, 512),
         (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512))
POOL_BEFORE = (5, 10, 17, 24)
TAPS = (2, 7, 14, 21, 28)
TAP_CHANNELS = (64, 128, 256, 512, 512)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)


def random_weights(seed: int = 0):
    """(vgg16_state, lin_state) with the packages' key names: convolution weights N(0, 2 / (9 Cin)), small random biases, lin >= 0."""
    g = torch.Generator().manual_seed(seed)
    vgg, lin = {}, {}
    for idx, cin, cout in CONVS:
        vgg[f"features.{idx}.weight"] = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
        vgg[f"features.{idx}.bias"] = 0.05 * torch.randn(cout, generator=g)
    for i, c in enumerate(TAP_CHANNELS):
        lin[f"lin{i}.model.1.weight"] = torch.rand((1, c, 1, 1), generator=g) / c
    return vgg, lin


def features(x, vgg_state, dtype):
    """x [N,3,H,W], already scaled -> the five tap tensors [N,C,h,w]"""
    taps = []
    for idx, _, _ in CONVS:
        if idx in POOL_BEFORE:
            x = F.max_pool2d(x, 2)
        x = F.relu(F.conv2d(x, vgg_state[f"features.{idx}.weight"].to(dtype), vgg_state[f"features.{idx}.bias"].to(dtype), padding=1))
        if idx in TAPS:
            taps.append(x)
    return taps


def scaling_layer(x, dtype):
    shift = torch.tensor(SHIFT, dtype=torch.float32, device=x.device).to(dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float32, device=x.device).to(dtype).view(1, 3, 1, 1)
    return (x - shift) / scale


def lpips_ref(in0, in1, vgg_state, lin_state, normalize=False, dtype=torch.float32):
    """in0, in1 [N,3,H,W] on the CPU -> [N,1,1,1] in `dtype`"""
    in0, in1 = in0.to(dtype), in1.to(dtype)
    if normalize:
        in0, in1 = 2 * in0 - 1, 2 * in1 - 1
    return distance(features(scaling_layer(in0, dtype), vgg_state, dtype), features(scaling_layer(in1, dtype), vgg_state, dtype), lin_state, dtype)


def distance(f0, f1, lin_state, dtype):
    """two results of features() -> [N,1,1,1]"""
    total = 0
    for i, (a, b) in enumerate(zip(f0, f1)):
        a = a / (torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True)) + 1e-10)
        b = b / (torch.sqrt(torch.sum(b ** 2, dim=1, keepdim=True)) + 1e-10)
        d = F.conv2d((a - b) ** 2, lin_state[f"lin{i}.model.1.weight"].to(dtype))
        total = total + d.mean([2, 3], keepdim=True)
    return total
