"""GPU: the step-level statement of tests/test_nonfinite_gpu.py's contract ("GradScaler skips the same
steps").  One +inf is injected into one optimizer step of the smallest model of tests/test_backbone_f16_gpu.py
(det_win_96x128) at one of five points, through hooks at boundaries that both paths call the same way:

  stem    the output of the SPM stem: a forward pre-hook on spm.conv2[0], the convolution that reads it
  mlp     the input of a block's MLP: a forward pre-hook on blocks[1].mlp
  msda    one injector's deformable-attention output: a forward hook on interactions[1].injector.attn
  msda_in the query that injector's deformable attention reads (from it the sampling offsets and the logits are made, so
          the deformable-attention kernels themselves meet non-finite locations and weights): a forward pre-hook on it
  grad    one element of the gradient of the last feature map: a tensor hook

(fused.linear(lin, x) does not call lin.__call__, so hooks on the Linear layers themselves would not fire on the default
path; the firings are counted and must be equal in both runs.)

The step runs once on the default path and once with every fused.ENABLED switch off and the attention on torch's math
statement, which is torch's path.  Under fp16 autocast with GradScaler(init_scale=512): whenever torch's path skips the
step (the scale halved after update() and every parameter bit-identical to before), the default path skips it too.
Under bf16 autocast without a scaler: whenever the loss or a parameter gradient is non-finite on torch's path, the loss
or a parameter gradient is non-finite on the default path."""
import pytest
import torch

from test_backbone_f16_gpu import _det_win_96x128

pytestmark = pytest.mark.gpu

INF = float('inf')
POINTS = ('stem', 'mlp', 'msda', 'msda_in', 'grad')


@pytest.fixture(scope='module', autouse=True)
def _fp32_math():
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    yield


@pytest.fixture(scope='module', autouse=True)
def _no_live_tuning():
    """The GEMM dispatcher in mode 0 (hipBLASLt's first heuristic answer, no candidate runs), as
    tests/test_gemm_f16_fp64_gpu.py.  With live tuning a problem that is first seen in the poisoned step has a reference
    product with NaN in it, every candidate fails the comparison (csrc/gemm.hip full_compare) and the call raises
    "no algorithm": an error, not a swallowed value, and the tuner's own question."""
    import _vah
    from test_gemm_f16_fp64_gpu import _env_tuning
    _vah.check(_vah.lib.vah_gemm_set_tuning(0, 32), 'gemm_set_tuning')
    yield
    _vah.check(_vah.lib.vah_gemm_set_tuning(*_env_tuning()), 'gemm_set_tuning')


def _poison(t):
    t = t.clone()
    t.view(-1)[t.numel() // 2 + 1] = INF
    return t


def _hooks(model, point, fired):
    """-> (module hook handles, tensor hook for the last feature map or None)"""
    def count():
        fired[point] = fired.get(point, 0) + 1

    def pre(mod, args):
        count()
        return (_poison(args[0]),) + tuple(args[1:])

    def post(mod, args, out):
        count()
        return _poison(out)

    def grad(g):
        count()
        return _poison(g)

    if point == 'stem':
        return [model.spm.conv2[0].register_forward_pre_hook(pre)], None
    if point == 'mlp':
        return [model.blocks[1].mlp.register_forward_pre_hook(pre)], None
    if point == 'msda_in':
        return [model.interactions[1].injector.attn.register_forward_pre_hook(pre)], None
    if point == 'msda':
        return [model.interactions[1].injector.attn.register_forward_hook(post)], None
    return [], grad


def _step(point, dtype, torch_path, monkeypatch):
    """one optimizer step with the injection -> dict(fired, loss_finite, grads_finite, skipped, scale)"""
    from vitadapter import fused, kernels
    with monkeypatch.context() as mp:
        if torch_path:
            for k in fused.ENABLED:
                mp.setitem(fused.ENABLED, k, False)
            mp.setitem(kernels.FLAGS, 'force_math_attention', True)
        torch.manual_seed(0)
        model, x = _det_win_96x128()
        model = model.cuda().train()
        x = x.cuda()
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        before = {k: p.detach().clone() for k, p in model.named_parameters()}
        amp = dtype == torch.float16
        scaler = torch.amp.GradScaler('cuda', init_scale=512., enabled=amp)
        fired = {}
        handles, grad_hook = _hooks(model, point, fired)
        try:
            with torch.autocast('cuda', dtype=dtype):
                outs = model(x)
            if grad_hook is not None:
                outs[-1].register_hook(grad_hook)
            g = torch.Generator(device='cuda').manual_seed(7)
            loss = sum((t.float() * torch.randn(t.shape, device='cuda', generator=g)).mean() for t in outs)
            scaler.scale(loss).backward()
            grads_finite = all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
            scaler.step(opt)
            scaler.update()
            torch.cuda.synchronize()
        finally:
            for h in handles:
                h.remove()
        same = all(torch.equal(p.detach(), before[k]) for k, p in model.named_parameters())
        return dict(fired=fired.get(point, 0), loss_finite=bool(torch.isfinite(loss)), grads_finite=grads_finite,
                    skipped=amp and same and scaler.get_scale() == 256., same=same, scale=scaler.get_scale() if amp else None)


@pytest.mark.parametrize('point', POINTS)
def test_grad_scaler_skips_the_steps_torch_skips(point, monkeypatch):
    ref = _step(point, torch.float16, True, monkeypatch)
    got = _step(point, torch.float16, False, monkeypatch)
    print('fp16 %s: torch path %r, default path %r' % (point, ref, got))
    assert ref['fired'] == got['fired'] >= 1, (ref['fired'], got['fired'])
    assert ref['skipped'], 'torch takes this step: the case asserts nothing (%r)' % (ref,)
    if ref['skipped']:
        assert got['skipped'], 'torch skips this step, the default path takes it: scale %r, parameters unchanged %r' % (
            got['scale'], got['same'])


@pytest.mark.parametrize('point', POINTS)
def test_bf16_step_is_non_finite_where_torchs_is(point, monkeypatch):
    ref = _step(point, torch.bfloat16, True, monkeypatch)
    got = _step(point, torch.bfloat16, False, monkeypatch)
    print('bf16 %s: torch path %r, default path %r' % (point, ref, got))
    assert ref['fired'] == got['fired'] >= 1, (ref['fired'], got['fired'])
    assert not (ref['loss_finite'] and ref['grads_finite']), 'torch\'s step is finite: the case asserts nothing (%r)' % (ref,)
    if not (ref['loss_finite'] and ref['grads_finite']):
        assert not (got['loss_finite'] and got['grads_finite']), 'torch\'s loss or gradients are non-finite, the default path\'s are all finite'
