"""The stub case of tests/golden/segmentor.npz (tools/gen_golden_segmentor.py) for the segmentor tests: the stub backbone
and head, the images and metas, rebuilt from the file's ``meta``.  Not a conftest and not a test module."""
import json
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'segmentor.npz')


class Attr:
    """a test_cfg that is an attribute object, not a dict"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class StubBackbone(nn.Module):
    def forward(self, img):
        return F.avg_pool2d(img, 4)


class StubHead(nn.Module):
    def __init__(self, weight, bias, loss_keys, align_corners=False):
        super().__init__()
        self.weight, self.bias = nn.Parameter(torch.as_tensor(weight).clone()), nn.Parameter(torch.as_tensor(bias).clone())
        self.num_classes = self.weight.shape[0]
        self.align_corners = align_corners
        self.loss_keys = loss_keys

    def forward_test(self, x, img_metas, test_cfg):
        return F.conv2d(x, self.weight, self.bias)

    def forward_train(self, x, img_metas, gt_semantic_seg, **kwargs):
        return {k: F.conv2d(x, self.weight, self.bias).mean() * (i + 1) for i, k in enumerate(self.loss_keys)}


class Case:
    def __init__(self):
        self.gold = np.load(GOLDEN)
        self.meta = json.loads(str(self.gold['meta']))
        self.views = self.meta['views']
        self.ori = tuple(self.meta['ori_shape'])

    def image(self, view, dtype=torch.float64, device='cpu'):
        h, w = view['hw']
        n = 3 * h * w
        return torch.cos(torch.arange(n, dtype=torch.float64) * 0.37 + view['j']).reshape(1, 3, h, w).to(device=device, dtype=dtype)

    def metas(self, view, **over):
        m = dict(ori_shape=self.ori, img_shape=tuple(view['img_shape']), flip=view['flip'], flip_direction=view['flip_direction'])
        m.update(over)
        return [m]

    def test_cfg(self, mode='slide', as_dict=False):
        kw = dict(mode=mode, crop_size=(self.meta['crop'],) * 2, stride=(self.meta['stride'],) * 2)
        return kw if as_dict else Attr(**kw)

    def build(self, cls, mode='slide', dtype=torch.float64, device='cpu', as_dict=False):
        head = StubHead(self.gold['head_weight'], self.gold['head_bias'], self.meta['loss_keys'])
        return cls(StubBackbone(), head, test_cfg=self.test_cfg(mode, as_dict)).to(device=device, dtype=dtype).eval()
