"""A stand-in for the reference's GSRegresser, for the decoder-glue module tests (test_upcat_module.py on the CPU, test_gpu_upcat.py on the GPU):
the regresser's member names and data flow with tiny widths and plain layers.  Its own forward is the unconverted one -- `up`, then torch.cat in two
stages, as the reference concatenates the two feature tensors of a level first."""
import torch
from torch import nn


class DepthEncoder(nn.Module):
    """Three levels at 1/2, 1/4 and 1/8 of the input's resolution (stride 3: 1/3, 1/9, 1/27, for a module whose `up` has a scale of 3)."""

    def __init__(self, dims, stride=2):
        super().__init__()
        self.l1 = nn.Sequential(nn.Conv2d(1, dims[0], 3, stride=stride, padding=1), nn.ReLU())
        self.l2 = nn.Sequential(nn.Conv2d(dims[0], dims[1], 3, stride=stride, padding=1), nn.ReLU())
        self.l3 = nn.Sequential(nn.Conv2d(dims[1], dims[2], 3, stride=stride, padding=1), nn.ReLU())

    def forward(self, x):
        a = self.l1(x)
        b = self.l2(a)
        return a, b, self.l3(b)


def _decoder(cin, cout):
    return nn.Sequential(nn.Conv2d(cin, cout, 3, padding=1), nn.ReLU(), nn.Conv2d(cout, cout, 1))


def _head(dim, cout, act=None):
    layers = [nn.Conv2d(dim, dim, 3, padding=1), nn.ReLU(), nn.Conv2d(dim, cout, 1)]
    return nn.Sequential(*(layers + ([act] if act is not None else [])))


class Regresser(nn.Module):
    RGB, DEPTH, DEC, HEAD = (3, 4, 5), (2, 3, 4), (4, 5, 6), 8      # channels per level: image features, depth features, decoders; the heads

    def __init__(self, up=None, stride=2, head=None):
        super().__init__()
        r, d, dec = self.RGB, self.DEPTH, self.DEC
        self.HEAD = self.HEAD if head is None else head       # (32: widths the head and 3x3 conversions of this package take)
        self.depth_encoder = DepthEncoder(d, stride)
        self.decoder3 = _decoder(r[2] + d[2], dec[2])
        self.decoder2 = _decoder(r[1] + d[1] + dec[2], dec[1])
        self.decoder1 = _decoder(r[0] + d[0] + dec[1], dec[0])
        self.up = nn.Upsample(scale_factor=2, mode="bilinear") if up is None else up
        self.out_conv = nn.Conv2d(dec[0] + 3 + 1, self.HEAD, 3, padding=1)
        self.out_relu = nn.ReLU(inplace=True)
        self.rot_head = _head(self.HEAD, 4)
        self.scale_head = _head(self.HEAD, 3, nn.Softplus(beta=100))
        self.opacity_head = _head(self.HEAD, 1, nn.Sigmoid())

    def forward(self, img, depth, img_feat):
        i1, i2, i3 = img_feat
        d1, d2, d3 = self.depth_encoder(depth)
        level3, level2, level1 = torch.cat([i3, d3], 1), torch.cat([i2, d2], 1), torch.cat([i1, d1], 1)
        x = self.decoder3(level3)
        x = self.decoder2(torch.cat([self.up(x), level2], 1))
        x = self.decoder1(torch.cat([self.up(x), level1], 1))
        x = self.out_relu(self.out_conv(torch.cat([self.up(x), img, depth], 1)))
        return nn.functional.normalize(self.rot_head(x), dim=1), torch.clamp_max(self.scale_head(x), 0.01), self.opacity_head(x)


def inputs(N=2, H=16, W=24, seed=0, device="cpu", dtype=torch.float32, stride=2):
    """img [N,3,H,W], depth [N,1,H,W] and the three image feature levels, seeded (H and W multiples of stride^3)."""
    g = torch.Generator().manual_seed(seed)
    new = lambda c, s: torch.randn(N, c, H // s, W // s, generator=g).to(device=device, dtype=dtype)
    img, depth = new(3, 1), new(1, 1)
    return img, depth, [new(c, s) for c, s in zip(Regresser.RGB, (stride, stride ** 2, stride ** 3))]
