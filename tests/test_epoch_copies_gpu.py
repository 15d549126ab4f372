"""GPU: the one-launch 16-bit parameter copies of a forward epoch (csrc/epoch_copies.hip, vitadapter/fused.py::_EpochCopies).

The toy model of tests/epoch_toy.py has one module of every kind the table writes jobs for, with +-inf, NaN, values beyond
fp16's range, subnormals and exact ties between two bf16 / fp16 neighbours planted in its weights.  Inside an epoch every
served copy must equal, bit for bit (NaN for NaN), the torch expression the per-use code makes with the switch off.  The
rest is the epoch contract: a `.data` write between two forwards is seen, a backward after a later forward still has the
copy of its own forward, a captured forward + backward replays with weights changed in place, and a capture that finds
no valid table takes the per-use path and is right all the same."""
import pytest
import torch

import epoch_toy
from vitadapter import fused, spm_nhwc

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(autouse=True)
def _switch_on():
    old = fused.ENABLED['epoch_copies']
    fused.ENABLED['epoch_copies'] = True
    yield
    fused.ENABLED['epoch_copies'] = old


def _model(special):
    """With the special values: the toy at its smallest, for the copies alone.  Without: 64-channel 3x3 convolutions, the
    narrowest the conv kernels run."""
    return epoch_toy.plant(epoch_toy.Toy(16 if special else 64).to(DEV), special=special)


@pytest.mark.parametrize('t16', [torch.bfloat16, torch.float16])
def test_served_copies_are_the_torch_expressions_bit_for_bit(t16):
    model = _model(True)
    want = epoch_toy.expected(model, t16)
    with torch.autocast('cuda', dtype=t16), fused.forward_epoch(model):
        got = epoch_toy.served(model, t16)
        # through the public lookups as well: a conv weight viewed as a matrix is served its parameter's copy
        w = model.patch.weight
        if t16 == torch.bfloat16:
            v = fused.BF16_COPIES.get(w.view(w.shape[0], -1), t16)
            assert v.data_ptr() == got['patch.weight'].data_ptr() and v.shape == (16, 192)
            core = fused.PAIR_CORE_COPIES.get(model.pair2.sampling_offsets, model.pair2.attention_weights, 3)
            assert core[0].data_ptr() == got['pair2.core_w'].data_ptr() and core[2][2].dtype == torch.int32
    torch.cuda.synchronize()
    assert set(got) == set(want)
    bases = {t.untyped_storage().data_ptr() for k, t in got.items() if t is not None and t.dtype == t16}
    assert len(bases) == 1, 'the 16-bit copies of one epoch live in one buffer'
    for k, w in want.items():
        epoch_toy.assert_same_bits(got[k], w, '%s (%s)' % (k, t16))
    # outside the epoch nothing is served
    assert all(t is None for t in epoch_toy.served(model, t16).values())


def test_switch_off_serves_no_layouts():
    model = _model(False)
    fused.ENABLED['epoch_copies'] = False
    with torch.autocast('cuda', dtype=torch.bfloat16), fused.forward_epoch(model):
        got = epoch_toy.served(model, torch.bfloat16)
    assert got['lin1.weight'] is not None and got['up'] is None and got['conv_a.w9'] is None and got['pair1.core_w'] is None
    assert got['fc.weight'] is None


def _inputs(seed=1):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    return dict(x=r(2, 32, 24), img=r(2, 3, 32, 32), tok=r(2, 64, 16), query=r(2, 16, 16),
                value=r(2, 16, 2, 32).to(torch.bfloat16), ref=torch.rand(1, 16, 1, 2, generator=g).to(DEV),
                shapes=torch.tensor([[4, 4]], device=DEV), lsi=torch.zeros(1, dtype=torch.long, device=DEV))


def _forward(model, ins, t16=torch.bfloat16):
    """Every consumer of the epoch's copies once; -> list of outputs (fp32)."""
    outs = []
    with torch.autocast('cuda', dtype=t16), fused.forward_epoch(model):
        outs.append(fused.linear(model.lin1, ins['x']))
        t = spm_nhwc.image_to_nhwc16(ins['img'], t16)
        t = spm_nhwc._Conv3x3.apply(t, model.conv_a.weight, 1)
        t = spm_nhwc._Conv3x3.apply(t, model.conv_b.weight, 2)                  # its input gradient reads the dgrad layout
        outs.append(t)
        planes = fused.conv1x1(model.fc, t.permute(0, 3, 1, 2).contiguous())
        outs.append(planes)
        up = fused.up_from_tokens(model.up, ins['tok'], 8, 8)
        assert up is not None
        outs.append(up)
        pe = fused.patch_embed(model.patch, ins['img'])
        assert pe is not None
        outs.append(pe[0])
        assert fused.msda_pair_core_ok(model.pair1, ins['query'], ins['value'], ins['ref'])
        outs.append(fused.msda_pair_core(model.pair1, ins['query'], ins['value'], ins['shapes'], ins['lsi'], ins['ref']))
    return [o.float() for o in outs]


def _loss(outs):
    return sum((o * o).mean() for o in outs)


def _grads(model):
    return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def _reference(model, ins):
    """The same forward + backward with the switch off: the per-use torch expressions."""
    fused.ENABLED['epoch_copies'] = False
    try:
        model.zero_grad(set_to_none=True)
        outs = _forward(model, ins)
        _loss(outs).backward()
        torch.cuda.synchronize()
        return [o.detach().clone() for o in outs], _grads(model)
    finally:
        fused.ENABLED['epoch_copies'] = True


def _assert_equal_runs(got, want, what):
    outs, grads = got
    wouts, wgrads = want
    for i, (o, w) in enumerate(zip(outs, wouts)):
        assert torch.equal(o, w), '%s: output %d differs' % (what, i)
    assert set(grads) == set(wgrads)
    for n in grads:
        assert torch.equal(grads[n], wgrads[n]), '%s: gradient of %s differs' % (what, n)


def test_forward_backward_equals_the_per_use_path_and_sees_data_writes():
    model, ins = _model(False), _inputs()
    want = _reference(model, ins)
    model.zero_grad(set_to_none=True)
    outs = _forward(model, ins)
    _loss(outs).backward()
    torch.cuda.synchronize()
    _assert_equal_runs(([o.detach() for o in outs], _grads(model)), want, 'first forward')
    # lin1 (2), conv_a, conv_b, fc.weight, up.weight, patch (2), pair1's two Linears (4): every consumer reached its parameter
    assert len(want[1]) == 12
    with torch.no_grad():                           # .data writes: no version bump, same storage - the table stays valid
        for p in model.parameters():
            p.data.mul_(1.5)
    table = model.__dict__[fused._EpochCopies.ATTR][(torch.bfloat16, ins['x'].device)]
    want2 = _reference(model, ins)
    model.zero_grad(set_to_none=True)
    outs2 = _forward(model, ins)
    assert model.__dict__[fused._EpochCopies.ATTR][(torch.bfloat16, ins['x'].device)] is table, 'the table was rebuilt'
    _loss(outs2).backward()
    torch.cuda.synchronize()
    _assert_equal_runs(([o.detach() for o in outs2], _grads(model)), want2, 'after the .data write')
    assert not torch.equal(outs2[0], outs[0])


def test_backward_after_a_later_forward_uses_its_own_copies():
    model, ins = _model(False), _inputs()
    want = _reference(model, ins)
    model.zero_grad(set_to_none=True)
    outs_a = _forward(model, ins)                   # forward A
    with torch.no_grad():
        for p in model.parameters():
            p.data.mul_(-2.0)
    outs_b = _forward(model, ins)                   # forward B on other weights: a new epoch, a new buffer
    _loss(outs_a).backward()                        # backward A
    torch.cuda.synchronize()
    _assert_equal_runs(([o.detach() for o in outs_a], _grads(model)), want, 'backward A after forward B')
    assert not torch.equal(outs_b[0], outs_a[0])


def _capture(model, ins):
    """Forward + backward of the toy model as one HIP graph -> (graph, outputs, parameter -> gradient buffer)."""
    graph = torch.cuda.CUDAGraph()
    model.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        outs = _forward(model, ins)
        _loss(outs).backward()
    return graph, outs, {n: p.grad for n, p in model.named_parameters() if p.grad is not None}


def test_captured_step_replays_with_weights_changed_in_place():
    model, ins = _model(False), _inputs()
    for _ in range(2):                              # warm-up: builds the table, tunes the GEMMs
        model.zero_grad(set_to_none=True)
        _loss(_forward(model, ins)).backward()
    torch.cuda.synchronize()
    calls = []
    real = fused._EpochCopies.build
    fused._EpochCopies.build = lambda self, *a: (calls.append(1), real(self, *a))[1]
    try:
        graph, outs, grads = _capture(model, ins)
    finally:
        fused._EpochCopies.build = real
    assert not calls, 'the capture rebuilt the table'
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(0.5).add_(0.01)
    graph.replay()
    torch.cuda.synchronize()
    got = ([o.detach().clone() for o in outs], {n: g.clone() for n, g in grads.items()})
    _assert_equal_runs(got, _reference(model, ins), 'replay after an in-place change')


def test_capture_without_a_valid_table_takes_the_per_use_path():
    model, ins = _model(False), _inputs()
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        _loss(_forward(model, ins)).backward()
    torch.cuda.synchronize()
    with torch.no_grad():                           # a new storage for one parameter: the table's addresses are stale
        model.lin1.weight.data = model.lin1.weight.data.clone()
    table = model.__dict__[fused._EpochCopies.ATTR][(torch.bfloat16, ins['x'].device)]
    assert not table.valid()
    graph, outs, grads = _capture(model, ins)
    assert model.__dict__[fused._EpochCopies.ATTR][(torch.bfloat16, ins['x'].device)] is table and not table.valid()
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(0.5).add_(0.01)
    graph.replay()
    torch.cuda.synchronize()
    got = ([o.detach().clone() for o in outs], {n: g.clone() for n, g in grads.items()})
    _assert_equal_runs(got, _reference(model, ins), 'replay of a capture without a table')
    model.zero_grad(set_to_none=True)
    _forward(model, ins)                            # the next eager forward rebuilds it
    assert model.__dict__[fused._EpochCopies.ATTR][(torch.bfloat16, ins['x'].device)].valid()
