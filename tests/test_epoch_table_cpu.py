"""CPU: the job table of vitadapter/fused.py::_EpochCopies, run by a torch model of csrc/epoch_copies.hip.

The table is built for the toy model of tests/epoch_toy.py on CPU tensors (a job holds an address; nothing here reads
through it: the address is mapped back to its parameter).  Every job is executed as include/vitadapter_hip_epoch.h
defines it - element e of the destination <-> (i0, i1, i2, i3), source offset sum i_k * s_k, zero beyond the source's
extents, torch's cast - and every view the epoch would hand out must then equal, bit for bit, the torch expression the
per-use code makes.  The chunk table must cover every element of every job exactly once, no destination may overlap
another, and no job may read outside its parameter."""
import pytest
import torch

import epoch_toy
from vitadapter import fused

CPU = torch.device('cpu')


def _run_table(tab):
    out16 = torch.full((tab.n16,), float('nan'), dtype=tab.dtype)
    out32 = torch.full((max(tab.n32, 8),), float('nan'), dtype=torch.float32)
    written16, written32 = torch.zeros(tab.n16, dtype=torch.int32), torch.zeros(max(tab.n32, 8), dtype=torch.int32)
    for row in tab.jobs.tolist():
        src, dst, n, d1, d2, d3, s0, s1, s2, s3, l0, l1, l2, l3, flags, src_elems = row
        owner = [p for p in tab.params if p.data_ptr() <= src < p.data_ptr() + 4 * p.numel()]
        assert len(owner) == 1 and (src - owner[0].data_ptr()) % 4 == 0
        p = owner[0]
        base = (src - p.data_ptr()) // 4
        assert src_elems == p.numel() - base and n % (d1 * d2 * d3) == 0
        e = torch.arange(n)
        i3, t = e % d3, e // d3
        i2, t = t % d2, t // d2
        i1, i0 = t % d1, t // d1
        off = i0 * s0 + i1 * s1 + i2 * s2 + i3 * s3
        inside = (i0 < l0) & (i1 < l1) & (i2 < l2) & (i3 < l3)
        assert int(off[inside].max()) < src_elems and int(off[inside].min()) >= 0, 'a job reads outside its parameter'
        if flags & 1:           # dense: the kernel reads src[e] without looking at dims, strides or extents
            assert bool(inside.all()) and torch.equal(off, e)
        vals = torch.where(inside, p.detach().reshape(-1)[(base + off).clamp(0, p.numel() - 1)], torch.zeros(()))
        if flags & 2:
            assert dst % 4 == 0 and dst + n <= tab.n32
            out32[dst:dst + n] = vals
            written32[dst:dst + n] += 1
        else:
            assert dst % 8 == 0 and dst + n <= tab.n16
            out16[dst:dst + n] = vals.to(tab.dtype)
            written16[dst:dst + n] += 1
    assert int(written16.max()) <= 1 and int(written32.max()) <= 1, 'two jobs write the same element'
    return out16, out32


def _check_chunks(tab):
    chunk = 2048
    jobs, chunks = tab.jobs.tolist(), tab.chunks.tolist()
    assert tab.chunks.dtype == torch.int32 and tab.jobs.dtype == torch.int64 and tab.nchunks == len(chunks)
    seen = {}
    for j, k in chunks:
        seen.setdefault(j, []).append(k)
    assert sorted(seen) == list(range(len(jobs)))
    for j, ks in seen.items():
        assert sorted(ks) == list(range((jobs[j][2] + chunk - 1) // chunk)), j


@pytest.mark.parametrize('t16', [torch.bfloat16, torch.float16])
def test_table_makes_every_copy(t16):
    model = epoch_toy.plant(epoch_toy.Toy())
    tab = fused.EPOCH_COPIES.build(model, t16, CPU)
    assert tab.valid() and tab.nchunks > 0
    _check_chunks(tab)
    out16, out32 = _run_table(tab)
    got = {}
    names = {id(p): n for n, p in model.named_parameters()}
    for s in tab.serve:
        if s[0] == 'plain':
            got[names[id(s[1])]] = out16[s[2]:s[2] + s[1].numel()].view(s[1].shape)
        elif s[0] == 'up':
            got['up'] = out16[s[2]:s[2] + s[1].numel()].view(s[3])
        elif s[0] == 'conv9':
            n = s[3][0] * s[3][1] * s[3][2]
            name = names[id(s[1])][:-len('.weight')]
            got[name + '.w9'], got[name + '.wt9'] = out16[s[2]:s[2] + n].view(s[3]), out16[s[4]:s[4] + n].view(s[5])
        else:
            a, b, ow, wshape, ob, perm = s[1:]
            name = names[id(a.weight)].split('.')[0]
            got[name + '.core_w'] = out16[ow:ow + wshape[0] * wshape[1]].view(wshape)
            got[name + '.core_b'] = out32[ob:ob + wshape[0]]
            assert torch.equal(perm[0], epoch_toy._pair_rows(getattr(model, name))) and perm[2].dtype == torch.int32
            assert torch.equal(perm[2].long(), perm[0]) and torch.equal(perm[1][perm[0]], torch.arange(wshape[0]))
    rename = {'pair1.sampling_offsets': 'pair1.a', 'pair1.attention_weights': 'pair1.b', 'pair2.sampling_offsets': 'pair2.a',
              'pair2.attention_weights': 'pair2.b'}
    for k in list(got):
        head = k.rsplit('.', 1)[0]
        if head in rename:
            got[rename[head] + '.' + k.rsplit('.', 1)[1]] = got.pop(k)
    want = epoch_toy.expected(model, t16)
    assert set(want) <= set(got), sorted(set(want) - set(got))
    for k, w in want.items():
        epoch_toy.assert_same_bits(got[k], w, '%s (%s)' % (k, t16))


def test_table_follows_its_parameters():
    """valid() compares data_ptr, shape and dtype: a .data write keeps the table, a replaced storage does not."""
    model = epoch_toy.plant(epoch_toy.Toy(), special=False)
    tab = fused.EPOCH_COPIES.build(model, torch.bfloat16, CPU)
    model.lin1.weight.data.mul_(2)
    assert tab.valid()
    model.lin1.weight.data = model.lin1.weight.data.clone()
    assert not tab.valid()


def test_no_table_no_epoch_on_cpu():
    """forward_epoch on a CPU model opens nothing (no live CUDA parameter) and the layouts are not served."""
    model = epoch_toy.Toy()
    with torch.autocast('cpu', dtype=torch.bfloat16), fused.forward_epoch(model):
        assert fused.BF16_COPIES.layout('up', model.up.weight, torch.bfloat16) is None
        assert fused.BF16_COPIES.epoch % 2 == 0
