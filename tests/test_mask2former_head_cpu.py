"""CPU: vitadapter.Mask2FormerHead against tests/golden/mask2former_head.npz (computed by the reference's own class, see
tools/gen_golden_mask2former_head.py): state-dict layout, constructor errors, and the fp32 forward and backward at the bounds
of tests/test_pixel_decoder_module.py::test_gpu_fp32_matches_golden (2e-4 outputs / 2e-4 input gradients / 3e-4 parameter
gradients, with its floors).  The helpers are shared with tests/test_mask2former_head_gpu.py."""
import copy
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'mask2former_head.npz')
PD_GOLD = os.path.join(ROOT, 'tests', 'golden', 'pixel_decoder.npz')


@pytest.fixture(scope='module')
def gold():
    g, pdg = np.load(GOLD), np.load(PD_GOLD)
    return g, pdg, json.loads(str(g['meta']))


def _grid(g, key):
    return torch.from_numpy(g[key + '_q'].astype(np.float32)) * float(g[key + '_scale'])


def gout(shape, j):
    n = int(np.prod(shape))
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.37 + j).reshape(tuple(shape)).float()


def build_model(g, pdg, meta, dev):
    from vitadapter import Mask2FormerHead
    m = Mask2FormerHead(**meta['config'])
    sd = {}
    for k, shape in meta['state_dict'].items():
        v = _grid(pdg, 'w_' + k[len('pixel_decoder.'):]) if k.startswith('pixel_decoder.') else _grid(g, 'w_' + k)
        sd[k] = 1.0 + v if (v.dim() == 1 and not k.endswith('bias')) else v
        assert list(v.shape) == shape, k
    m.load_state_dict(sd)
    return m.to(dev)


def feats_of(pdg, dev):
    return [_grid(pdg, 'base_feat%d' % i).to(dev).requires_grad_(True) for i in range(4)]


def _digest(t):
    a = t.detach().to(torch.float64).flatten().cpu().numpy()
    return np.array([a.sum(), (a * np.cos(np.arange(a.size, dtype=np.float64) * 0.61803398875)).sum()], dtype=np.float64)


def check_digest(what, t, want, tol):
    """tests/test_pixel_decoder_module.py::_check_digest"""
    got = _digest(t)
    bound = tol * max(1.0, want[3])
    assert np.abs(got - want[:2]).max() <= bound, (what, got, want, bound)
    assert abs(float(t.detach().abs().max()) - want[2]) <= tol * max(1.0, want[2]), (what, float(t.detach().abs().max()), want[2])
    assert abs(float(t.detach().double().abs().sum()) - want[3]) <= bound, (what, float(t.detach().double().abs().sum()), want[3])


class LogitTap:
    """records the mask logits every forward_head hands to the next layer"""

    def __init__(self, model):
        self.logits = []
        inner = model.forward_head

        def tapped(*a, **k):
            out = inner(*a, **k)
            self.logits.append(out[2].detach())
            return out
        model.forward_head = tapped


def check_forward_backward(g, pdg, meta, dev, tol_out, tol_g, tol_gp):
    m = build_model(g, pdg, meta, dev)
    feats = feats_of(pdg, dev)
    tap = LogitTap(m)
    cls_preds, mask_preds = m(feats)
    L = meta['layers']
    assert len(cls_preds) == len(mask_preds) == L + 1 and len(tap.logits) == L + 1
    # before anything is compared: every mask logit a layer consumes has the golden's sign, no element excluded
    for i in range(L):
        want = torch.from_numpy(g['l%d_logits' % i])
        got = tap.logits[i].cpu()
        assert got.shape == want.shape and got.dtype == torch.float32
        assert bool(((got < 0) == (want < 0)).all()), 'layer %d consumes another mask than the golden' % i
        assert float(want.abs().min()) >= meta['guard'] * meta['d'][i]
    assert meta['all_excluded_rows']
    for i, n, q in meta['all_excluded_rows']:
        assert bool((tap.logits[i][n, q] < 0).all()), 'the all-excluded row of the golden is not all-excluded here'
    outs = list(cls_preds) + list(mask_preds)
    for j, o in enumerate(outs):
        name = ('cls_pred%d' % j) if j <= L else ('mask_pred%d' % (j - L - 1))
        w = g[name]
        assert tuple(o.shape) == w.shape, (name, o.shape, w.shape)
        assert np.abs(o.detach().float().cpu().numpy() - w).max() <= tol_out, (name, np.abs(o.detach().float().cpu().numpy() - w).max())
    sum((o.float() * gout(o.shape, j).to(dev)).sum() for j, o in enumerate(outs)).backward()
    step = meta['step']
    for i, f in enumerate(feats):
        w = g['gfeat%d_sample' % i]
        got = f.grad.float().cpu().flatten()[::step].numpy()
        assert np.abs(got - w).max() <= tol_g * max(1.0, np.abs(w).max()), (i, np.abs(got - w).max())
        check_digest(('gfeat', i), f.grad, g['gfeat%d_digest' % i], tol_g)
    n = 0
    for k, p in m.named_parameters():
        check_digest(k, p.grad if p.grad is not None else torch.zeros_like(p), g['gp_' + k], tol_gp)
        n += 1
    assert n == len(meta['state_dict'])


def test_state_dict_table_equals_the_goldens(gold):
    from vitadapter import Mask2FormerHead
    g, pdg, meta = gold
    m = Mask2FormerHead(**meta['config'])
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == meta['state_dict']
    keys = set(meta['state_dict'])
    for k in ('transformer_decoder.layers.2.attentions.0.attn.in_proj_weight', 'transformer_decoder.layers.0.attentions.1.attn.out_proj.bias',
              'transformer_decoder.layers.1.ffns.0.layers.0.0.weight', 'transformer_decoder.layers.1.ffns.0.layers.1.bias',
              'transformer_decoder.layers.0.norms.2.weight', 'transformer_decoder.post_norm.bias', 'query_embed.weight',
              'query_feat.weight', 'level_embed.weight', 'cls_embed.weight', 'mask_embed.0.weight', 'mask_embed.4.bias',
              'pixel_decoder.mask_feature.weight'):
        assert k in keys, k
    assert not any(k.startswith('decoder_input_projs') for k in keys)
    cfg = copy.deepcopy(meta['config'])
    cfg['enforce_decoder_input_project'] = True
    m2 = Mask2FormerHead(**cfg)
    assert m2.state_dict()['decoder_input_projs.2.weight'].shape == (64, 64, 1, 1)
    m2.init_weights()
    assert float(m2.decoder_input_projs[0].bias.detach().abs().max()) == 0.0
    assert m.loss_cls == meta['config']['loss_cls'] and m.train_cfg is None and m.num_classes == 5


def test_constructor_errors(gold):
    from vitadapter import Mask2FormerHead
    _, _, meta = gold

    def cfg(**edit):
        c = copy.deepcopy(meta['config'])
        for path, v in edit.items():
            d = c
            keys = path.split('__')
            for k in keys[:-1]:
                d = d[k]
            d[keys[-1]] = v
        return c
    Mask2FormerHead(**cfg())
    with pytest.raises(ValueError, match='operation_order'):
        Mask2FormerHead(**cfg(transformer_decoder__transformerlayers__operation_order=('self_attn', 'norm', 'cross_attn', 'norm', 'ffn', 'norm')))
    with pytest.raises(ValueError, match='ffn_cfgs'):
        Mask2FormerHead(**cfg(transformer_decoder__transformerlayers__ffn_cfgs__act_cfg=dict(type='GELU')))
    with pytest.raises(ValueError, match='SinePositionalEncoding'):
        Mask2FormerHead(**cfg(positional_encoding=dict(type='LearnedPositionalEncoding', num_feats=32)))
    with pytest.raises(ValueError, match='enforce_decoder_input_project'):
        Mask2FormerHead(**cfg(transformer_decoder__transformerlayers__attn_cfgs__embed_dims=128,
                              transformer_decoder__transformerlayers__ffn_cfgs__embed_dims=128))


def _patch_oracle(monkeypatch):
    """the deformable attention of the pixel decoder has no CPU kernels: the torch expression of oracle/msda.py stands in, as
    in tests/test_pixel_decoder_module.py"""
    import ops.modules.ms_deform_attn as mod
    from oracle import msda as oracle_msda

    class _OracleFunction:
        @staticmethod
        def apply(value, shapes, lsi, loc, attn, step):
            return oracle_msda.core_torch(value, shapes, loc, attn)
    monkeypatch.setattr(mod, 'MSDeformAttnFunction', _OracleFunction)


def test_cpu_fp32_matches_golden(gold, monkeypatch):
    g, pdg, meta = gold
    _patch_oracle(monkeypatch)
    check_forward_backward(g, pdg, meta, 'cpu', 2e-4, 2e-4, 3e-4)
