"""CPU: the three entry points of the fused MSDeformAttn core that take reference points per image
(include/vitadapter_hip.h: vah_msda_fused_forward_nref, vah_msda_fused_backward_nref, vah_msda_fused_backward_tiled_nref -
the existing signatures plus one int64 ref_batch directly after ref_levels).  Every call here is answered by the
host-side validation before anything touches a device, as in tests/test_abi_errors_cpu.py."""
import os
import re

import pytest

import _vah

lib = _vah.lib
OK, E_NULL, E_SHAPE = 0, -1, -2
P = 4096           # a non-null, 16-byte aligned fake pointer: never dereferenced by a rejected call
NAMES = ('vah_msda_fused_forward_nref', 'vah_msda_fused_backward_nref', 'vah_msda_fused_backward_tiled_nref')
S, M, D, L, PTS = 64, 2, 32, 1, 4


def _err():
    return lib.vah_last_error().decode()


def _call(name, ref_batch, N=2, Lq=8, ref=P):
    """One call with valid fake operands: bf16 values, fp32 contiguous offsets / logits, ref_levels 1."""
    if name == 'vah_msda_fused_forward_nref':
        return lib.vah_msda_fused_forward_nref(P, 1, P, P, P, P, 0, 0, 0, ref, 1, ref_batch, N, S, M, D, L, Lq, PTS, P, None)
    if name == 'vah_msda_fused_backward_nref':
        return lib.vah_msda_fused_backward_nref(P, 1, P, P, P, P, 0, ref, 1, ref_batch, P, N, S, M, D, L, Lq, PTS, P, P, P, None)
    return lib.vah_msda_fused_backward_tiled_nref(P, 1, P, P, P, P, 0, 0, 0, ref, 1, ref_batch, P, N, S, M, D, L, Lq, PTS, P, 1,
                                                  P, P, 1, 0, 0, P, 1 << 30, None)


@pytest.mark.parametrize('name', NAMES)
def test_symbols_are_exported_and_declared(name):
    assert name in _vah.EXPORTS and hasattr(lib, name)
    header = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'vitadapter_hip.h')
    with open(header) as f:
        text = f.read()
    decl = re.search(r'\bint %s\(([^;]*)\);' % name, text)
    assert decl, name + ' is not declared in include/vitadapter_hip.h'
    assert re.search(r'int64_t ref_levels,\s*int64_t ref_batch,', decl.group(1)), 'ref_batch directly after ref_levels'


def test_adding_symbols_does_not_move_the_abi_version():
    assert lib.vah_abi_version() == 37 == _vah.ABI_VERSION


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('ref_batch', [0, 3, -1])
def test_ref_batch_must_be_one_or_n(name, ref_batch):
    assert _call(name, ref_batch, N=2) == E_SHAPE
    assert 'ref_batch' in _err() and name in _err(), _err()


@pytest.mark.parametrize('name', NAMES)
def test_null_ref_and_empty_calls(name):
    assert _call(name, 2, N=2, ref=None) == E_NULL
    assert 'null' in _err()
    assert _call(name, 1, N=2, ref=None) == E_NULL
    # N * Lq * M == 0: nothing to do is not an error, whatever the pointers
    assert _call(name, 2, N=2, Lq=0, ref=None) == OK
    assert _call(name, 1, N=2, Lq=0, ref=None) == OK
    assert _call(name, 0, N=0, ref=None) == OK
    # ... but a ref_batch that is neither 1 nor N still is one
    assert _call(name, 3, N=2, Lq=0, ref=None) == E_SHAPE
