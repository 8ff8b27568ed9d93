"""The parameters of LPIPS (AlexNet, v0.1): the five convolutions of torchvision's `alexnet().features` and the five bias-free
1x1 "lin" layers of the `lpips` package, under the names both files use.

    features.{0,3,6,8,10}.{weight,bias}      torchvision's alexnet state dict (its classifier.* entries are ignored)
    lin{0..4}.model.1.weight                 lpips' weights/v0.1/alex.pth, shape (1, C, 1, 1)

`LpipsAlexWeights.random(seed)` gives a seeded network of the same shapes -- what the tests and the benchmark run, since the
metric's arithmetic does not depend on the values --, `from_files` / `from_state_dicts` read the real files, `find()` looks for them
under $CTRLV_MODEL_ROOT/lpips/.  Nothing is downloaded.  `plan.LpipsPlan(weights, device)` runs the network on the HIP kernels
(csrc/lpips.hip); `split_weight_columns` restates, in torch, the split weight rows those kernels contract against."""
import math
import os

import torch

# (features index, Cin, Cout, kernel, stride, padding) of the five convolutions; a max-pool (3, stride 2) follows the ReLU of the
# first two
CONVS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1))
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
ALEXNET_FILES = ("alexnet.safetensors", "alexnet.pth", "alexnet-owt-7be5be79.pth")
LIN_FILES = ("alex.safetensors", "alex.pth")


def conv_keys():
    return [f"features.{i}.{p}" for i, *_ in CONVS for p in ("weight", "bias")]


def lin_keys():
    return [f"lin{l}.model.1.weight" for l in range(len(CONVS))]


def _load_file(path):
    if str(path).endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(str(path))
    return torch.load(str(path), map_location="cpu", weights_only=True)


def split_weight_columns(weight, order, dtype):
    """weight (N, C, k, k) fp32 -> (N, 3 Kp) of `dtype` = whi | wlo | whi with whi = rne(w), wlo = rne(w - whi), in the column
    order of the matching im2col: order 0 (c, ky, kx), order 1 (ky, kx, c); Kp = k k C rounded up to a multiple of 64, the
    padding columns zero.  What ctrlv_lpips_pack_weight writes, bit for bit."""
    w = weight.detach().float()
    N, C, k, _ = w.shape
    cols = w.reshape(N, C * k * k) if order == 0 else w.permute(0, 2, 3, 1).reshape(N, k * k * C)
    K = cols.shape[1]
    Kp = (K + 63) // 64 * 64
    full = torch.zeros(N, Kp, dtype=torch.float32, device=w.device)
    full[:, :K] = cols
    hi = full.to(dtype)
    lo = (full - hi.float()).to(dtype)
    return torch.cat([hi, lo, hi], dim=1)


class LpipsAlexWeights:
    """A state dict {name: fp32 tensor} with exactly `conv_keys() + lin_keys()`, checked for shape."""

    def __init__(self, tensors):
        self.tensors = {}
        for (i, cin, cout, k, _, _), l in zip(CONVS, range(len(CONVS))):
            for name, shape in ((f"features.{i}.weight", (cout, cin, k, k)), (f"features.{i}.bias", (cout,)),
                                (f"lin{l}.model.1.weight", (1, cout, 1, 1))):
                if name not in tensors:
                    raise KeyError(f"LpipsAlexWeights: missing tensor '{name}'")
                t = tensors[name].detach().float().contiguous()
                if tuple(t.shape) != shape:
                    raise ValueError(f"LpipsAlexWeights: '{name}' has shape {tuple(t.shape)}, expected {shape}")
                self.tensors[name] = t

    def state_dict(self):
        return dict(self.tensors)

    def conv(self, l):
        i = CONVS[l][0]
        return self.tensors[f"features.{i}.weight"], self.tensors[f"features.{i}.bias"]

    def lin(self, l):
        return self.tensors[f"lin{l}.model.1.weight"].reshape(-1)

    @classmethod
    def random(cls, seed=0):
        """He-scaled convolutions (std sqrt(2 / fan_in)), bias 0.1 N(0, 1), lin = U(0, 2 / C) >= 0."""
        g = torch.Generator().manual_seed(int(seed))
        t = {}
        for l, (i, cin, cout, k, _, _) in enumerate(CONVS):
            t[f"features.{i}.weight"] = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * k * k))
            t[f"features.{i}.bias"] = 0.1 * torch.randn(cout, generator=g)
            t[f"lin{l}.model.1.weight"] = torch.rand(1, cout, 1, 1, generator=g) * (2.0 / cout)
        return cls(t)

    @classmethod
    def from_state_dicts(cls, alexnet, lin):
        """alexnet: torchvision's `alexnet` state dict; lin: the state dict of lpips' weights/v0.1/alex.pth."""
        t = {}
        for name in conv_keys():
            if name not in alexnet:
                raise KeyError(f"LpipsAlexWeights: the alexnet state dict has no '{name}'")
            t[name] = alexnet[name]
        for name in lin_keys():
            if name not in lin:
                raise KeyError(f"LpipsAlexWeights: the lin state dict has no '{name}'")
            t[name] = lin[name]
        return cls(t)

    @classmethod
    def from_files(cls, alexnet_path, lin_path):
        """Either file as .pth (torch.load(weights_only=True)) or .safetensors."""
        return cls.from_state_dicts(_load_file(alexnet_path), _load_file(lin_path))

    @staticmethod
    def find(root=None):
        """(alexnet_path, lin_path) under <root or $CTRLV_MODEL_ROOT>/lpips/, or None when either is not there."""
        root = root or os.environ.get("CTRLV_MODEL_ROOT")
        if not root:
            return None
        d = os.path.join(root, "lpips")
        found = []
        for names in (ALEXNET_FILES, LIN_FILES):
            hit = next((os.path.join(d, n) for n in names if os.path.isfile(os.path.join(d, n))), None)
            if hit is None:
                return None
            found.append(hit)
        return tuple(found)


__all__ = ["LpipsAlexWeights", "split_weight_columns", "CONVS", "SHIFT", "SCALE", "conv_keys", "lin_keys"]
