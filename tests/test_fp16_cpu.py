"""CPU-side checks of the fp16 inference mode: the reference-made goldens are consistent
with a restatement of the specification built from the oracle's functions, the packed fp16 weight order against a
numpy statement, option plumbing, and the new host-side queries.  No kernel is launched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import tecogan_pytorch_amd  # noqa: F401
from tecogan_pytorch_amd import _lib as L
from tecogan_pytorch_amd import ops
from tecogan_pytorch_amd.models.networks import FRNet, define_generator
from procedural_weights import generator_state_dict, smooth_clip
import fp16_fixture as FX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- golden self-consistency -----------------------------------------------------------------------------------

@pytest.mark.parametrize('name', FX.CLIPS)
def test_golden_is_reproduced_by_the_oracle_restatement(name):
    """The specification restated with the oracle's functions (float64 accumulation in the fp16 layers) against the
    reference-made `spec` frames: the golden pins the specification, not the hooks it was made with.  Frame 0 runs on
    the zero state -- nothing in front of SRNet reaches it -- so the restatement must land well inside the golden's
    implementation noise there (it differs in the fp32 HR stage's last bits only).  From frame 1 on the oracle's fp32
    FNet / warp are not bit-identical to the reference modules', and a last-bit change of SRNet's input flips fp16
    roundings like any other summation order does: there the restatement is one more equally valid implementation and
    gets the margin every such comparison in this project gets, twice the noise."""
    g = FX.load(name)
    s, deg = g['scale'], g['degradation']
    sd = generator_state_dict(scale=s, degradation=deg)
    clip = smooth_clip(g['t'], 3, g['h'], g['w'], seed=g['seed'])
    mine = FX.infer_fp16(sd, clip, s, deg, wide=True)
    assert mine.shape[0] == g['t'] and g['u8'].shape == (g['t'], s * g['h'], s * g['w'], 3)
    assert FX.rel_l2(mine[0], g['hr_first']) <= g['noise_rel_l2'][0]
    assert FX.rel_l2(mine[-1], g['hr_last']) <= 2 * g['noise_rel_l2'][-1]
    from oracle import tecogan_oracle as O
    for i in range(g['t']):
        share, mx = FX.u8_diff(O.float32_to_uint8(mine[i]).transpose(1, 2, 0), g['u8'][i])
        assert share <= (1 if i == 0 else 2) * g['noise_u8_share'][i] and mx <= 1, (i, share, mx)


@pytest.mark.parametrize('name', FX.CLIPS)
def test_golden_figures_are_what_the_issue_measured(name):
    """The yardsticks are the reference's own: implementation noise and the fp16-vs-fp32 distance are of one size
    (1e-4 class, never more than one uint8 level), i.e. far from a bf16-like rounding (8x larger)."""
    g = FX.load(name)
    assert g['noise_u8_max'].max() <= 1 and g['fp32_u8_max'].max() <= 1
    assert 1e-5 < g['noise_rel_l2'].min() and g['noise_rel_l2'].max() < 4e-4
    assert g['fp32_rel_l2'].max() < 4e-4
    assert g['noise_u8_share'].max() < 0.04
    assert os.path.getsize(os.path.join(FX.HERE, f'fp16_{name}.npz')) < (1 << 20)


# ---- weight rounding / packing ---------------------------------------------------------------------------------

@pytest.mark.parametrize('transposed,cin,cout', [(False, 64, 64), (False, 51, 64), (False, 15, 64), (True, 64, 64)])
def test_pack_index_against_numpy_statement(transposed, cin, cout):
    """ops.f16_pack_index is the host statement of the packed order (the GPU test compares the pack kernel with it):
    checked here against an explicit loop over the MFMA A-operand map (lane l holds W[row l % 16][k = 8 (l / 16) + j])."""
    idx = ops.f16_pack_index(transposed, cin, cout)
    assert idx.shape == (18 * 4 * 64 * 8,) and idx.shape[0] == L.lib().tg_conv3x3_f16_packed_halves(cin, cout)
    rng = np.random.default_rng(0)
    w = rng.standard_normal((cin, cout, 3, 3) if transposed else (cout, cin, 3, 3)).astype(np.float32)
    packed = np.where(idx >= 0, w.reshape(-1)[np.maximum(idx, 0)], 0).astype(np.float16)
    wk = w.transpose(1, 0, 2, 3) if transposed else w              # (cout, cin, ky, kx)
    seen = 0
    for ks in (0, 1, 7, 17):
        for ct in range(4):
            for lane in (0, 5, 16, 37, 63):
                for j in range(8):
                    co, ci, tap = 16 * ct + lane % 16, 32 * (ks % 2) + 8 * (lane // 16) + j, ks // 2
                    exp = np.float16(wk[co, ci, tap // 3, tap % 3]) if (co < cout and ci < cin) else np.float16(0)
                    assert packed[((ks * 4 + ct) * 64 + lane) * 8 + j] == exp
                    seen += 1
    assert seen == 4 * 4 * 5 * 8
    # every real weight appears exactly once, the rest is padding
    real = idx[idx >= 0]
    assert real.size == cin * cout * 9 and np.array_equal(np.sort(real), np.arange(cin * cout * 9))


def test_fp16_rounding_is_nearest_even():
    """The rounding the specification (and the fixture) uses: ties go to the even mantissa."""
    x = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 65504.0, 2.0 ** -25])
    assert FX.r16(x).tolist() == [1.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -10, 65504.0, 0.0]


# ---- option plumbing -------------------------------------------------------------------------------------------

def _opt(**gen):
    return {'scale': 4, 'dataset': {'degradation': {'type': 'BD'}},
            'model': {'generator': dict({'name': 'FRNet', 'in_nc': 3, 'out_nc': 3, 'nf': 64, 'nb': 10}, **gen)}}


def test_precision_option_plumbing():
    assert FRNet(3, 3, 64, 10, 'BD', 4).precision == 'fp32'
    assert define_generator(_opt()).precision == 'fp32'
    assert define_generator(_opt(precision='fp32')).precision == 'fp32'
    assert define_generator(_opt(precision='fp16')).precision == 'fp16'
    with pytest.raises(ValueError):
        define_generator(_opt(precision='bf16'))
    with pytest.raises(ValueError):
        FRNet(3, 3, 64, 10, 'BD', 4, precision='half')
    net = FRNet(3, 3, 64, 10, 'BD', 4, precision='fp16')
    with pytest.raises(ValueError):
        net.precision = 'fp64'
    assert net.precision == 'fp16'                       # a refused value changes nothing


def test_precision_is_not_a_parameter_and_is_in_the_plan_key():
    a, b = FRNet(3, 3, 64, 10, 'BD', 4), FRNet(3, 3, 64, 10, 'BD', 4, precision='fp16')
    assert set(a.state_dict()) == set(b.state_dict())
    b.load_state_dict(generator_state_dict(scale=4, degradation='BD'), strict=True)
    k32, k16 = a._plan_cache_key(1, 32, 48, 'cuda:0', False), b._plan_cache_key(1, 32, 48, 'cuda:0', False)
    assert k32 != k16 and k32[:-1] == k16[:-1] and k16[-1] == 'fp16'
    b._plan['sentinel'] = object()
    b.precision = 'fp16'                                 # same value: plans are kept
    assert 'sentinel' in b._plan
    b.precision = 'fp32'                                 # switched: plans are dropped
    assert b._plan == {} and b._plan_cache_key(1, 32, 48, 'cuda:0', False) == k32


def test_yml_round_trip_and_cli_override(tmp_path):
    import yaml
    from tecogan_pytorch_amd import main as M
    opt = M.default_opt()
    assert 'precision' not in opt['model']['generator']              # absent = fp32
    opt['model']['generator']['precision'] = 'fp16'
    (tmp_path / 'test.yml').write_text(yaml.dump(opt))
    back = yaml.load((tmp_path / 'test.yml').read_text(), Loader=yaml.FullLoader)
    assert define_generator(back).precision == 'fp16'
    args = M.parse_args(['--mode', 'profile', '--precision', 'fp16'])
    assert args.precision == 'fp16' and M.parse_args(['--mode', 'profile']).precision is None
    with pytest.raises(SystemExit):
        M.parse_args(['--mode', 'profile', '--precision', 'bf16'])


# ---- C ABI: host-side queries and refusals ---------------------------------------------------------------------

def test_header_declares_the_new_symbols_and_the_library_exports_them():
    text = open(os.path.join(ROOT, 'include', 'tecogan_hip.h')).read()
    handle = ctypes.CDLL(L.LIB_PATH)
    for s in ('tg_conv3x3_f16_supported', 'tg_conv3x3_f16_packed_halves', 'tg_conv3x3_f16_act_halves',
              'tg_conv3x3_f16_pack_weights', 'tg_conv3x3_f16_pack_input', 'tg_conv3x3_f16_fwd', 'tg_convt3x3s2_f16_fwd',
              'tg_frnet_f16_workspace_bytes', 'tg_frnet_plan_set_precision', 'tg_frnet_plan_precision'):
        assert s + '(' in text, s
        assert hasattr(handle, s), s
        assert s in L.SIGNATURES
    assert 'TG_PREC_F16' in text and L.PREC_F16 == 1 and L.PREC_F32 == 0


def test_shape_and_size_queries_without_a_device():
    lib = L.lib()
    sup = lib.tg_conv3x3_f16_supported
    assert sup(1, 64, 64, 134, 320) and sup(3, 64, 64, 37, 53) and sup(1, 64, 64, 3, 3) and sup(2, 64, 64, 144, 180)
    assert not sup(0, 64, 64, 134, 320) and not sup(1, 51, 64, 134, 320) and not sup(1, 64, 32, 134, 320)
    assert not sup(1, 64, 64, 0, 320) and not sup(1, 64, 64, 134, -1) and not sup(1, 128, 128, 16, 16)
    assert lib.tg_conv3x3_f16_packed_halves(64, 64) == 18 * 4 * 64 * 8
    assert lib.tg_conv3x3_f16_packed_halves(51, 64) == 18 * 4 * 64 * 8           # K padded with zero weights
    assert lib.tg_conv3x3_f16_packed_halves(65, 64) == 0 and lib.tg_conv3x3_f16_packed_halves(64, 0) == 0
    assert lib.tg_conv3x3_f16_act_halves(3, 37, 53) == 3 * 37 * 53 * 64
    assert lib.tg_conv3x3_f16_act_halves(0, 37, 53) == -1
    ok = L.FrnetCfg(3, 3, 64, 10, 4, 1, 1, 134, 320, 0)
    nbytes = lib.tg_frnet_f16_workspace_bytes(ctypes.byref(ok))
    assert nbytes >= 22 * 18 * 4 * 64 * 8 * 2 + 2 * 134 * 320 * 64 * 2 and nbytes % 16 == 0
    assert lib.tg_frnet_f16_workspace_bytes(ctypes.byref(L.FrnetCfg(3, 3, 32, 10, 4, 1, 1, 134, 320, 0))) == 0   # nf != 64
    assert lib.tg_frnet_f16_workspace_bytes(ctypes.byref(L.FrnetCfg(3, 3, 64, 10, 4, 1, 1, 134, 320, 1))) == 0   # FNet-only
    assert lib.tg_frnet_f16_workspace_bytes(ctypes.byref(L.FrnetCfg(4, 3, 64, 10, 4, 1, 1, 134, 320, 0))) == 0   # bad cfg


def test_entry_points_refuse_bad_arguments_with_codes():
    lib = L.lib()
    assert lib.tg_conv3x3_f16_fwd(None, None, None, None, None, 1, 64, 64, 8, 8, 0, None) == -2
    assert b'null' in lib.tg_last_error_string()
    assert lib.tg_convt3x3s2_f16_fwd(None, None, None, None, 0, 1, 64, 64, 8, 8, 0, None) == -2
    assert lib.tg_conv3x3_f16_pack_weights(None, 64, 64, 0, None, None) == -2
    assert lib.tg_conv3x3_f16_pack_input(None, 0, 3, None, 0, 48, None, 1, 8, 8, None) == -2
    # aligned, non-null host addresses: the shape / enum checks come before any launch
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 255) & ~255
    x, y, wp, b = a, a + 1024, a + 2048, a + 3072
    assert lib.tg_conv3x3_f16_fwd(x, wp, b, None, y, 1, 32, 64, 8, 8, 0, None) == -1          # cin != 64
    assert lib.tg_conv3x3_f16_fwd(x, wp, b, None, x, 1, 64, 64, 8, 8, 0, None) == -2          # y aliases x
    assert lib.tg_conv3x3_f16_fwd(x, wp, b, None, y, 1, 64, 64, 8, 8, 2, None) == -2          # LeakyReLU: not offered
    assert lib.tg_conv3x3_f16_fwd(x + 2, wp, b, None, y, 1, 64, 64, 8, 8, 0, None) == -2      # alignment
    assert lib.tg_convt3x3s2_f16_fwd(x, wp, b, y, 64 * 4 * 64, 1, 64, 64, 8, 8, 3, None) == -2
    assert lib.tg_convt3x3s2_f16_fwd(x, wp, b, y, 16, 1, 64, 64, 8, 8, 1, None) == -1         # y_nstride too small
    assert lib.tg_conv3x3_f16_pack_weights(x, 65, 64, 0, y, None) == -1
    assert lib.tg_conv3x3_f16_pack_input(x, 0, 3, wp, 0, 62, y, 1, 8, 8, None) == -1          # 3 + 62 > 64
    assert lib.tg_frnet_plan_set_precision(None, 1, None, 0, None) == -2
    assert lib.tg_frnet_plan_precision(None) == 0
