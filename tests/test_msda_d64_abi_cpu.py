"""CPU: heads of 64 channels in the fused MSDeformAttn core (include/vitadapter_hip.h) and the ViT-Adapter-S presets.

D = 64 is taken by vah_msda_fused_forward[_nref], vah_msda_fused_forward_win and vah_msda_fused_backward_tiled[_nref];
the atomic vah_msda_fused_backward[_nref] stays at D = 32; every other width is VAH_E_UNSUPPORTED.  Every call here is
answered by the host-side validation before anything touches a device (fake, aligned pointers that are never
dereferenced), as in tests/test_abi_errors_cpu.py."""
import pytest
import torch

import _vah

lib = _vah.lib
OK, E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3, -4
P = 4096           # a non-null, 16-byte aligned fake pointer
N, S, M, L, LQ, PTS = 2, 64, 2, 1, 8, 4
F32, BF16, F16 = 0, 1, 2


def _err():
    return lib.vah_last_error().decode()


def _tiled(name, D, v, p, gv, gp, ws_bytes, os_=0, ls=0, dos=0, dls=0):
    head = (P, v, P, P, P, P, p, os_, ls, P, 1)
    tail = (P, N, S, M, D, L, LQ, PTS, P, gv, P, P, gp, dos, dls, P, ws_bytes, None)
    if name.endswith('_nref'):
        return getattr(lib, name)(*head, 1, *tail)
    return getattr(lib, name)(*head, *tail)


def _forward(name, D, v, p, os_=0, ls=0):
    head = (P, v, P, P, P, P, p, os_, ls, P, 1)
    tail = (N, S, M, D, L, LQ, PTS, P, None)
    if name.endswith('_nref'):
        return getattr(lib, name)(*head, 1, *tail)
    return getattr(lib, name)(*head, *tail)


def _forward_win(D, v, p, ws_bytes, os_=0, ls=0):
    return lib.vah_msda_fused_forward_win(P, v, P, P, P, P, p, os_, ls, P, N, S, M, D, LQ, PTS, 5, P, ws_bytes, 0, P, None)


def _atomic(name, D, v, p):
    head = (P, v, P, P, P, P, p, P, 1)
    tail = (P, N, S, M, D, L, LQ, PTS, P, P, P, None)
    if name.endswith('_nref'):
        return getattr(lib, name)(*head, 1, *tail)
    return getattr(lib, name)(*head, *tail)


TILED = ('vah_msda_fused_backward_tiled', 'vah_msda_fused_backward_tiled_nref')
FORWARD = ('vah_msda_fused_forward', 'vah_msda_fused_forward_nref')
ATOMIC = ('vah_msda_fused_backward', 'vah_msda_fused_backward_nref')
FORMS = [(F32, F32, F32, F32), (BF16, BF16, BF16, BF16), (BF16, F32, BF16, BF16), (BF16, F32, F32, F32), (F32, BF16, F32, BF16),
         (F16, F16, F16, F16)]


def test_supported_widths():
    for levels in (1, 3, 4):
        assert lib.vah_msda_fused_supported(64, levels, 4) == 1
        assert lib.vah_msda_fused_supported(32, levels, 4) == 1
    for D in (48, 96, 128):
        for levels in (1, 3, 4):
            assert lib.vah_msda_fused_supported(D, levels, 4) == 0
    assert lib.vah_msda_fused_supported(64, 2, 4) == 0 and lib.vah_msda_fused_supported(64, 3, 8) == 0


@pytest.mark.parametrize('name', ATOMIC)
def test_atomic_backward_stays_at_32_channels(name):
    assert _atomic(name, 64, BF16, BF16) == E_UNSUPPORTED, _err()
    assert 'D == 32' in _err() and 'tiled' in _err()
    assert _atomic(name, 64, F32, F32) == E_UNSUPPORTED, _err()


@pytest.mark.parametrize('name', TILED)
def test_tiled_backward_sizes_its_workspace_by_head_slices(name):
    """vah_msda_tile_ws_bytes counts 32-channel head slices: a D = 64 call needs the bound for 2 M, and a workspace sized
    for M is refused with the too-small error; every dtype form gets as far as that check."""
    for_m, for_2m = lib.vah_msda_tile_ws_bytes(N, S, M, L, LQ, PTS), lib.vah_msda_tile_ws_bytes(N, S, 2 * M, L, LQ, PTS)
    assert 0 < for_m < for_2m
    for v, p, gv, gp in FORMS:
        assert _tiled(name, 64, v, p, gv, gp, for_m) == E_SHAPE, ((v, p, gv, gp), _err())
        assert 'workspace too small' in _err()
        assert _tiled(name, 64, v, p, gv, gp, for_2m - 1) == E_SHAPE, ((v, p, gv, gp), _err())
        assert 'workspace too small' in _err()
        # D = 32 is held to the bound for M, as before
        assert _tiled(name, 32, v, p, gv, gp, for_m - 1) == E_SHAPE, _err()
    # with the right size the next host-side check answers: a null workspace pointer is not what is passed here, so a
    # misaligned offsets stride is used to stop the call before any launch
    assert _tiled(name, 64, BF16, BF16, BF16, BF16, for_2m, 20, 20, 20, 20) == E_ALIGN, _err()


def test_forward_entry_points_take_64_channels():
    """No workspace in the gather forward: the last host-side check behind D and the dtype codes is the one on the row
    strides; the window forward reaches its workspace check."""
    for name in FORWARD:
        assert _forward(name, 64, BF16, BF16, 18, 18) == E_ALIGN, _err()
        assert 'strides' in _err()
        assert _forward(name, 64, F16, F16, 18, 18) == E_ALIGN, _err()
    need = lib.vah_msda_win_ws_bytes(S, LQ)
    assert _forward_win(64, BF16, F32, need - 1) == E_SHAPE, _err()
    assert 'workspace too small' in _err()
    assert _forward_win(64, F16, F16, need - 1) == E_SHAPE, _err()


@pytest.mark.parametrize('D', [48, 96, 128, 16])
def test_other_widths_are_refused(D):
    need = lib.vah_msda_tile_ws_bytes(N, S, 4 * M, L, LQ, PTS)
    for name in TILED:
        assert _tiled(name, D, BF16, BF16, BF16, BF16, need) == E_UNSUPPORTED, (name, _err())
    for name in FORWARD:
        assert _forward(name, D, BF16, BF16) == E_UNSUPPORTED, (name, _err())
    assert _forward_win(D, BF16, BF16, lib.vah_msda_win_ws_bytes(S, LQ)) == E_UNSUPPORTED, _err()
    for name in ATOMIC:
        assert _atomic(name, D, BF16, BF16) == E_UNSUPPORTED, (name, _err())


@pytest.mark.parametrize('v,p', [(F16, BF16), (F16, F32), (BF16, F16), (F32, F16)])
def test_fp16_with_another_type_is_still_refused_at_64_channels(v, p):
    need = lib.vah_msda_tile_ws_bytes(N, S, 2 * M, L, LQ, PTS)
    for name in TILED:
        assert _tiled(name, 64, v, p, v, p, need) == E_UNSUPPORTED, (name, _err())
        assert 'fp16' in _err()
    for name in FORWARD:
        assert _forward(name, 64, v, p) == E_UNSUPPORTED, (name, _err())
    assert _forward_win(64, v, p, lib.vah_msda_win_ws_bytes(S, LQ)) == E_UNSUPPORTED, _err()


def test_abi_version_and_exports_are_unchanged():
    assert lib.vah_abi_version() == 37 == _vah.ABI_VERSION
    assert len(_vah.EXPORTS) == 122 and len(_vah.SIGNATURES) == 79


def test_host_layer_sizes_the_workspace_by_head_slices():
    from ops.functions import ms_deform_attn_fused as mf
    assert mf.tile_ws_bytes(N, S, M, 64, L, LQ, PTS) == lib.vah_msda_tile_ws_bytes(N, S, 2 * M, L, LQ, PTS)
    assert mf.tile_ws_bytes(N, S, M, 32, L, LQ, PTS) == lib.vah_msda_tile_ws_bytes(N, S, M, L, LQ, PTS)


@pytest.mark.parametrize('name', ['small_seg', 'small_det'])
def test_small_presets_build_with_64_channel_deformable_heads(name):
    """ViT-Adapter-S (upernet_deit_adapter_small_512_160k_ade20k.py:10-26, mask_rcnn_deit_adapter_small_fpn_3x_coco.py:
    11-29): embed_dim 384, 6 deformable heads, deform_ratio 1.0 -> d_value 384, heads of 64 channels.  The state-dict keys
    of the adapter parts are those of the tiny preset (same depth, interaction indexes and module tree in the reference,
    upernet_deit_adapter_tiny_512_160k_ade20k.py:10-26) with 384-wide shapes."""
    from ops.modules import MSDeformAttn
    from vitadapter.backbones.vit_adapter import PRESETS, build_preset
    kw = PRESETS[name]
    assert (kw['embed_dim'], kw['depth'], kw['num_heads'], kw['drop_path_rate']) == (384, 12, 6, 0.2)
    assert (kw['deform_num_heads'], kw['deform_ratio'], kw['n_points']) == (6, 1.0, 4)
    if name == 'small_seg':
        assert kw['flavour'] == 'seg' and kw['window_attn'] == [False] * 12 and kw['window_size'] == [None] * 12
    else:
        assert kw['flavour'] == 'det' and kw['window_attn'] == [True, True, False] * 4
        assert kw['window_size'] == [14, 14, None] * 4
    model = build_preset(name)
    attns = [m for m in model.modules() if isinstance(m, MSDeformAttn)]
    assert len(attns) == 4 + 4 + 2          # an injector and an extractor per interaction, two extra extractors at the end
    for a in attns:
        assert a.n_heads == 6 and a.value_proj.out_features == 384 and a.value_proj.out_features // a.n_heads == 64
        assert a.n_levels in (1, 3) and a.n_points == 4
    sd = model.state_dict()
    adapter = ('level_embed', 'spm.', 'interactions.', 'up.', 'norm1.', 'norm2.', 'norm3.', 'norm4.')
    keys = {k for k in sd if k.startswith(adapter)}
    tiny = {k for k in build_preset('tiny_seg').state_dict() if k.startswith(adapter)}
    assert keys == tiny and len(keys) > 100
    assert tuple(sd['level_embed'].shape) == (3, 384)
    assert tuple(sd['interactions.0.injector.attn.value_proj.weight'].shape) == (384, 384)
    assert tuple(sd['interactions.0.injector.attn.sampling_offsets.weight'].shape) == (6 * 3 * 4 * 2, 384)
    assert tuple(sd['interactions.0.extractor.attn.sampling_offsets.weight'].shape) == (6 * 1 * 4 * 2, 384)
    assert tuple(sd['interactions.3.extra_extractors.1.attn.output_proj.weight'].shape) == (384, 384)
    assert isinstance(sd['spm.fc1.weight'], torch.Tensor) and sd['spm.fc1.weight'].shape[0] == 384
