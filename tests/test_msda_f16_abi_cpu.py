"""CPU: dtype code 2 (fp16) of the fused MSDeformAttn core (include/vitadapter_hip.h).  It is accepted in ONE form -
value / out / grad_out / grad_value and offsets / logits / d_offsets / d_logits all fp16 - by the existing forward entry
points and the tiled backward; every other use of it is VAH_E_UNSUPPORTED.  Every call here is answered by the host-side
validation before anything touches a device (fake, aligned pointers that are never dereferenced), as in
tests/test_abi_errors_cpu.py; the CPU tier also pins the inputs of tests/test_msda_f16_fp64_gpu.py."""
import pytest
import torch

import _vah
from oracle import msda_fused as mfo

lib = _vah.lib
OK, E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3, -4
P = 4096           # a non-null, 16-byte aligned fake pointer
N, S, M, D, L, LQ, PTS = 2, 64, 2, 32, 1, 8, 4
F32, BF16, F16 = 0, 1, 2


def _err():
    return lib.vah_last_error().decode()


def _tiled(name, v, p, gv, gp, ws_bytes, os_=0, ls=0, dos=0, dls=0):
    head = (P, v, P, P, P, P, p, os_, ls, P, 1)
    tail = (P, N, S, M, D, L, LQ, PTS, P, gv, P, P, gp, dos, dls, P, ws_bytes, None)
    if name.endswith('_nref'):
        return getattr(lib, name)(*head, 1, *tail)
    return getattr(lib, name)(*head, *tail)


def _forward(name, v, p, os_=0, ls=0):
    head = (P, v, P, P, P, P, p, os_, ls, P, 1)
    tail = (N, S, M, D, L, LQ, PTS, P, None)
    if name.endswith('_nref'):
        return getattr(lib, name)(*head, 1, *tail)
    return getattr(lib, name)(*head, *tail)


def _forward_win(v, p, ws_bytes, os_=0, ls=0):
    return lib.vah_msda_fused_forward_win(P, v, P, P, P, P, p, os_, ls, P, N, S, M, D, LQ, PTS, 5, P, ws_bytes, 0, P, None)


def _atomic(name, v, p):
    head = (P, v, P, P, P, P, p, P, 1)
    tail = (P, N, S, M, D, L, LQ, PTS, P, P, P, None)
    if name.endswith('_nref'):
        return getattr(lib, name)(*head, 1, *tail)
    return getattr(lib, name)(*head, *tail)


TILED = ('vah_msda_fused_backward_tiled', 'vah_msda_fused_backward_tiled_nref')
FORWARD = ('vah_msda_fused_forward', 'vah_msda_fused_forward_nref')
ATOMIC = ('vah_msda_fused_backward', 'vah_msda_fused_backward_nref')


@pytest.mark.parametrize('name', TILED)
def test_tiled_backward_takes_the_fp16_form(name):
    """Code 2 in the accepted form gets as far as the workspace check: one byte too few is the workspace error, not
    VAH_E_UNSUPPORTED.  (This fails on a library without the fp16 form.)"""
    need = lib.vah_msda_tile_ws_bytes(N, S, M, L, LQ, PTS)
    assert need > 0
    assert _tiled(name, F16, F16, F16, F16, need - 1) == E_SHAPE, _err()
    assert 'workspace too small' in _err()
    # row-strided fp16 operands: rows of 3 L P + 8 halves are 8-byte aligned and accepted ...
    assert _tiled(name, F16, F16, F16, F16, need - 1, 20, 20, 20, 20) == E_SHAPE, _err()
    assert 'workspace too small' in _err()
    # ... rows that are not, are not
    assert _tiled(name, F16, F16, F16, F16, need - 1, 18, 18, 20, 20) == E_ALIGN, _err()


def test_window_forward_takes_the_fp16_form():
    need = lib.vah_msda_win_ws_bytes(S, LQ)
    assert need > 0
    assert _forward_win(F16, F16, need - 1) == E_SHAPE, _err()
    assert 'workspace too small' in _err()
    assert _forward_win(F16, F16, need - 1, 20, 20) == E_SHAPE, _err()
    assert _forward_win(F16, F16, need, 18, 18) == E_ALIGN, _err()


@pytest.mark.parametrize('name', FORWARD)
def test_forward_takes_the_fp16_form(name):
    """No workspace here: the last host-side check behind the dtype codes is the one on the row strides."""
    assert _forward(name, F16, F16, 18, 18) == E_ALIGN, _err()
    assert 'strides' in _err()


@pytest.mark.parametrize('v,p', [(3, 3), (3, 0), (0, 3), (2, 3), (-1, 0), (4, 4)])
def test_other_codes_are_refused(v, p):
    need = lib.vah_msda_tile_ws_bytes(N, S, M, L, LQ, PTS)
    for name in TILED:
        assert _tiled(name, v, p, v, p, need) == E_UNSUPPORTED, (name, _err())
    for name in FORWARD:
        assert _forward(name, v, p) == E_UNSUPPORTED, (name, _err())
    assert _forward_win(v, p, lib.vah_msda_win_ws_bytes(S, LQ)) == E_UNSUPPORTED, _err()
    for name in ATOMIC:
        assert _atomic(name, v, p) == E_UNSUPPORTED, (name, _err())


@pytest.mark.parametrize('v,p', [(F16, BF16), (F16, F32), (BF16, F16), (F32, F16)])
def test_fp16_mixed_with_another_type_is_refused(v, p):
    need = lib.vah_msda_tile_ws_bytes(N, S, M, L, LQ, PTS)
    for name in TILED:
        assert _tiled(name, v, p, v, p, need) == E_UNSUPPORTED, (name, _err())
        assert 'fp16' in _err()
    for name in FORWARD:
        assert _forward(name, v, p) == E_UNSUPPORTED, (name, _err())
    assert _forward_win(v, p, lib.vah_msda_win_ws_bytes(S, LQ)) == E_UNSUPPORTED, _err()


@pytest.mark.parametrize('gv,gp', [(F32, F16), (F16, F32), (BF16, F16), (F16, BF16), (F32, F32), (BF16, BF16)])
def test_fp16_operands_take_fp16_gradients_only(gv, gp):
    need = lib.vah_msda_tile_ws_bytes(N, S, M, L, LQ, PTS)
    for name in TILED:
        assert _tiled(name, F16, F16, gv, gp, need) == E_UNSUPPORTED, (name, _err())


@pytest.mark.parametrize('v,p,gv,gp', [(BF16, BF16, F16, BF16), (BF16, BF16, BF16, F16), (F32, F32, F16, F32), (BF16, F32, BF16, F16)])
def test_fp16_gradients_of_other_operands_are_refused(v, p, gv, gp):
    need = lib.vah_msda_tile_ws_bytes(N, S, M, L, LQ, PTS)
    for name in TILED:
        assert _tiled(name, v, p, gv, gp, need) == E_UNSUPPORTED, (name, _err())


@pytest.mark.parametrize('name', ATOMIC)
def test_atomic_backward_refuses_fp16(name):
    """Its grad_value is fp32: there is no atomic fp16 backward."""
    assert _atomic(name, F16, F16) == E_UNSUPPORTED, _err()
    assert 'fp16' in _err()


def test_bf16_and_fp32_forms_still_reach_the_workspace_check():
    need = lib.vah_msda_tile_ws_bytes(N, S, M, L, LQ, PTS)
    for v, p, gv, gp in [(F32, F32, F32, F32), (BF16, BF16, BF16, BF16), (BF16, F32, BF16, BF16), (BF16, F32, F32, F32), (F32, BF16, F32, BF16)]:
        assert _tiled(TILED[0], v, p, gv, gp, need - 1) == E_SHAPE, ((v, p, gv, gp), _err())
    # their offsets rows keep the 16-byte rule
    assert _tiled(TILED[0], BF16, BF16, BF16, BF16, need - 1, 20, 20, 20, 20) == E_ALIGN, _err()


def test_abi_version_is_unchanged():
    assert lib.vah_abi_version() == 37 == _vah.ABI_VERSION


def test_host_layer_knows_the_code_and_the_switch():
    from ops.functions import ms_deform_attn_fused as mf
    from vitadapter import fused
    assert mf._DT == {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
    assert fused.ENABLED['fp16_msda'] is True


# the cases of tests/test_msda_f16_fp64_gpu.py that compare d_offsets under oracle.msda_fused.smooth_mask
F16_CASES = ['ext_ragged', 'inj_ragged', 'four_levels', 'shared_lists', 'wide_rows', 'borders', 'many_tiles']


@pytest.mark.parametrize('case', F16_CASES)
def test_fp16_offsets_leave_most_samples_off_the_kinks(case):
    """fp16 offsets sit on a coarse grid (2^-8 px between 4 and 8 px) and land on integer pixel coordinates far more
    often than fp32 ones: the mask of the fp64 test still has to keep more than half of the samples (oracle check())."""
    inp = mfo.inputs(case, 'F4')
    inp.offsets = inp.offsets.to(torch.float16)
    keep = float(mfo.smooth_mask(inp).mean())
    assert keep > 0.5, keep
