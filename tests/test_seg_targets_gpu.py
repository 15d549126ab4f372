"""GPU: the target kernels of csrc/seg_target.hip against tests/seg_targets_ref.py, through the ctypes ABI and through
fused.seg_targets, each case as uint8 and as int64.  Everything is an integer: every comparison is exact.

The cases are those of the golden (tests/seg_targets_ref.py).  'odd' lies in a buffer with row stride 17 whose first label is one
element past the buffer's start (uint8: an odd address; int64: off the 16-byte boundary), so heads and tails of rows take the
scalar loads and H * W = 91 takes the byte-store form of the mask launch; 'ranges' has four workgroup ranges an image, the last one
partial, and 16-byte stores (12576 = 16 * 786).  Every output buffer is filled with 0xFF before the call."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_targets_ref as ref  # noqa: E402
import test_mask2former_loss_cpu as loss_helpers  # noqa: E402

from vitadapter import fused  # noqa: E402

pytestmark = pytest.mark.gpu
_vah = fused._vah
lib = _vah.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'seg_targets.npz'))
MAPS = ref.case_maps()
TABLES = {None: None, 'mapillary': GOLD['mapillary_table'], 'reduce_zero': ref.reduce_zero_table()}
ROWS = ('seg_target_scan', 'seg_target_finish', 'seg_target_masks')
DTYPES = [torch.uint8, torch.int64]
_WANT = {}


def dev():
    return torch.device('cuda:0')


def want_of(case):
    if case not in _WANT:
        name, ignore, remap = ref.CASES[case]
        _WANT[case] = ref.targets(MAPS[name], ignore, TABLES[remap])
    return _WANT[case]


def place(m, case, dtype):
    """the map on the device; 'odd' strided and one element off the start of its buffer"""
    t = torch.from_numpy(m).to(dtype)
    N, H, W = t.shape
    if case != 'odd':
        return t.to(dev())
    buf = torch.full((1 + N * H * (W + 4),), 77, dtype=dtype)           # 77 is in no map: a read outside a row would show
    view = buf[1:].view(N, H, W + 4)[:, :, :W]
    view.copy_(t)
    out = buf.to(dev())[1:].view(N, H, W + 4)[:, :, :W]
    assert out.stride() == (H * (W + 4), W + 4, 1) and out.data_ptr() % 16 == out.element_size()
    return out


def table_of(remap):
    return None if TABLES[remap] is None else torch.from_numpy(TABLES[remap]).to(dev())


def abi(t, ignore, table):
    """the three launches through ctypes -> (dict like ref.targets, labels (N, 256), slot (N, 256), out-of-range flag)"""
    N, H, W = t.shape
    code = {torch.int64: 0, torch.uint8: 1}[t.dtype]
    nbytes = lib.vah_segtgt_ws_bytes(N, H, W)
    assert nbytes > 0
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=dev())
    labels = torch.full((N, 256), -1 << 40, dtype=torch.int64, device=dev())
    slot = torch.full((N, 256), -7, dtype=torch.int32, device=dev())
    meta = torch.full((N + 2,), -7, dtype=torch.int32, device=dev())
    tp = None if table is None else table.data_ptr()
    stream = _vah.raw_stream(dev())
    _vah.check(lib.vah_segtgt_scan(t.data_ptr(), code, t.stride(0), t.stride(1), N, H, W, ignore, tp, labels.data_ptr(), slot.data_ptr(),
                                   meta.data_ptr(), ws.data_ptr(), nbytes, stream), 'vah_segtgt_scan')
    host = meta.cpu().tolist()
    offsets, flag = host[:N + 1], host[N + 1]
    G = offsets[N]
    masks = torch.full((G + 1, H, W), 255, dtype=torch.uint8, device=dev())          # one plane more: it must stay 0xFF
    image_of = torch.full((G + 1,), -7, dtype=torch.int32, device=dev())
    out_labels = torch.full((G + 1,), -7, dtype=torch.int64, device=dev())
    _vah.check(lib.vah_segtgt_masks(t.data_ptr(), code, t.stride(0), t.stride(1), N, H, W, tp, slot.data_ptr(), labels.data_ptr(),
                                    meta.data_ptr(), G, masks.data_ptr(), image_of.data_ptr(), out_labels.data_ptr(), stream),
               'vah_segtgt_masks')
    torch.cuda.synchronize()
    assert bool((masks[G] == 255).all()) and int(image_of[G]) == -7 and int(out_labels[G]) == -7
    got = dict(masks=masks[:G].cpu().numpy(), labels=out_labels[:G].cpu().numpy(), image_of=image_of[:G].cpu().numpy(),
               counts=[b - a for a, b in zip(offsets, offsets[1:])], offsets=offsets)
    return got, labels.cpu().numpy(), slot.cpu().numpy(), flag


def equal(got, want):
    for k in ('masks', 'labels', 'image_of'):
        g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
        assert g.dtype == want[k].dtype and g.shape == want[k].shape and np.array_equal(g, want[k]), k
    offsets = got['offsets'].cpu().tolist() if torch.is_tensor(got['offsets']) else got['offsets']
    assert got['counts'] == want['counts'] and offsets == want['offsets']


def as_dict(t):
    assert isinstance(t, fused.SegTargets) and all(type(c) is int for c in t.counts)
    return dict(masks=t.masks, labels=t.labels, image_of=t.image_of, counts=t.counts, offsets=t.offsets)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', sorted(ref.CASES))
def test_abi_matches_the_rule(case, dtype):
    name, ignore, remap = ref.CASES[case]
    want = want_of(case)
    t = place(MAPS[name], case, dtype)
    got, labels, slot, flag = abi(t, ignore, table_of(remap))
    assert flag == 0
    equal(got, want)
    # labels [N][256]: ascending, -1 past the count; slot [N][256]: the global index of a present value, else -1
    o = want['offsets']
    for n in range(t.shape[0]):
        mine = want['labels'][o[n]:o[n + 1]]
        assert labels[n].tolist() == mine.tolist() + [-1] * (256 - len(mine))
        expect = np.full(256, -1, dtype=np.int32)
        expect[mine] = np.arange(o[n], o[n + 1])
        assert np.array_equal(slot[n], expect)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', sorted(ref.CASES))
def test_fused_matches_the_rule_on_and_off(case, dtype):
    name, ignore, remap = ref.CASES[case]
    t = place(MAPS[name], case, dtype)
    table = table_of(remap)
    _vah.prof_enable(True, 'seg_target')
    on = fused.seg_targets(t, ignore, table)
    rows = _vah.prof_report()
    _vah.prof_enable(False)
    for row in ROWS:                                            # the kernel route; no target: nothing for launch three to write
        assert rows.get(row, dict(calls=0))['calls'] == (0 if row == 'seg_target_masks' and not sum(on.counts) else 1), rows
    equal(as_dict(on), want_of(case))
    keep = fused.ENABLED['seg_targets']
    fused.ENABLED['seg_targets'] = False
    try:
        _vah.prof_enable(True, 'seg_target')
        off = fused.seg_targets(t, ignore, table)
        rows = _vah.prof_report()
        _vah.prof_enable(False)
    finally:
        fused.ENABLED['seg_targets'] = keep
    assert not any(row in rows for row in ROWS), rows
    equal(as_dict(off), want_of(case))
    assert off.masks.device == on.masks.device == t.device


def test_out_of_range_sets_the_flag_and_takes_the_torch_route():
    m = ref.OUT_OF_RANGE
    want = ref.targets(m, 255)
    assert want['labels'].tolist() == [-1, 0, 3, 300, 0] and want['counts'] == [4, 1]
    t = torch.from_numpy(m).to(dev())
    got, labels, slot, flag = abi(t, 255, None)
    assert flag == 1
    # what is in range is still ranked, what is not has indexed nothing
    assert got['counts'] == [2, 1] and got['labels'].tolist() == [0, 3, 0]
    assert np.array_equal(got['masks'], np.stack([m[0] == 0, m[0] == 3, m[1] == 0]).astype(np.uint8))
    _vah.prof_enable(True, 'seg_target')
    pending = fused.seg_targets_begin(t, 255)
    first = _vah.prof_report()
    _vah.prof_enable(False)
    assert first['seg_target_scan']['calls'] == 1 and first['seg_target_finish']['calls'] == 1 and 'seg_target_masks' not in first
    _vah.prof_enable(True, 'seg_target')
    res = pending.finish()                                      # the second pass: torch, none of the three rows
    second = _vah.prof_report()
    _vah.prof_enable(False)
    assert not any(row in second for row in ROWS), second
    equal(as_dict(res), want)
    clean = torch.from_numpy(np.where((m < 0) | (m > 255), 3, m)).to(dev())       # and the flag does not stick
    equal(as_dict(fused.seg_targets(clean, 255)), ref.targets(clean.cpu().numpy(), 255))


@pytest.mark.parametrize('dtype', DTYPES)
def test_begin_finish_split_with_other_work_between(dtype):
    t = place(MAPS['ranges'], 'ranges', dtype)
    a = fused.seg_targets_begin(t, 255)
    b = fused.seg_targets_begin(t[:1], 0)                       # a second handle in flight: its own pinned buffer
    x = torch.randn(512, 512, device=dev())
    for _ in range(4):
        x = x @ x * 1e-3
    other = place(MAPS['odd'], 'odd', dtype)
    c = fused.seg_targets(other, 255)
    rb, ra = b.finish(), a.finish()
    assert bool(torch.isfinite(x).all())
    equal(as_dict(ra), want_of('ranges'))
    equal(as_dict(rb), ref.targets(MAPS['ranges'][:1], 0))
    equal(as_dict(c), want_of('odd'))
    assert a.finish() is ra
    side = torch.cuda.Stream()
    d = fused.seg_targets_begin(t, 255)
    with torch.cuda.stream(side):
        rd = d.finish()                                         # finished on another stream: it waits for the event
    side.synchronize()
    equal(as_dict(rd), want_of('ranges'))


def test_empty_inputs():
    for shape in ((0, 4, 4), (2, 0, 4), (2, 4, 0)):
        r = fused.seg_targets(torch.zeros(shape, dtype=torch.uint8, device=dev()))
        assert tuple(r.masks.shape) == (0,) + shape[1:] and r.counts == [0] * shape[0] and r.offsets.tolist() == [0] * (shape[0] + 1)


def test_real_composition_trains_from_the_label_map():
    import test_segmentor_gpu as seg_helpers
    seg, meta = seg_helpers._real_segmentor()
    gen = torch.Generator().manual_seed(3)
    img = torch.randn(2, 3, 64, 64, generator=gen).to(dev())
    rng = np.random.RandomState(9)
    gt = rng.randint(0, meta['things'] + meta['stuff'], size=(2, 4, 4)).repeat(16, axis=1).repeat(16, axis=2).astype(np.int64)
    gt[0, 5:20, 7:30] = 255
    gt[1, :, :] = np.where(gt[1] > 1, 1, gt[1])
    want = ref.targets(gt, 255)
    assert min(want['counts']) >= 1 and want['counts'][0] != want['counts'][1]
    head, seen = seg.decode_head, []
    keep = head.loss
    head.loss = lambda *a: (seen.append(a[2]), keep(*a))[1]
    seg.train()
    _vah.prof_enable(True, 'seg_target')
    with torch.autocast('cuda', dtype=torch.bfloat16):
        losses = seg.forward_train(img, [None, None], torch.from_numpy(gt).to(dev()))
    rows = _vah.prof_report()
    _vah.prof_enable(False)
    assert all(rows[row]['calls'] == 1 for row in ROWS), rows
    assert len(seen) == 1
    equal(as_dict(seen[0]), want)
    gold_meta = json.loads(str(GOLD['meta']))
    assert [k[len('decode.'):] for k in losses] == gold_meta['loss_keys'] == meta['loss_keys']
    assert all(k.startswith('decode.') and bool(torch.isfinite(v)) for k, v in losses.items())
    sum(losses.values()).backward()
    grads = [p.grad for p in seg.parameters() if p.grad is not None]
    assert len(grads) > 50 and all(bool(torch.isfinite(g_).all()) for g_ in grads)
