"""The fp16 inference mode on the GPU: every layer kernel against torch float64 on identical
inputs with a derived bound, the whole SRNet body teacher-forced, whole clips against the reference-made goldens
(triangulated against the reference's own implementation noise), plan = layers bit for bit, and nothing leaking
into the fp32 path or into training.  No bound in this file is fitted to what the kernels give."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from procedural_weights import generator_state_dict, smooth_clip  # noqa: E402
import fp16_fixture as FX  # noqa: E402


@pytest.fixture(scope='module')
def ops():
    import tecogan_pytorch_amd.ops as ops_
    return ops_


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _h(t):
    """values exactly representable in fp16, kept in fp32"""
    return t.to(torch.float16).to(torch.float32)


def _nhwc16(x_nchw):
    """fp32 NCHW (fp16-representable) -> fp16 channels-last on the device"""
    return x_nchw.permute(0, 2, 3, 1).contiguous().to(torch.float16).cuda()


def _nchw(y_nhwc16):
    return y_nhwc16.cpu().to(torch.float64).permute(0, 3, 1, 2)


def _body_weights(scale=4, deg='BD', key='srnet.resblocks.3.conv.0'):
    sd = generator_state_dict(scale=scale, degradation=deg)
    return sd, sd[key + '.weight'].clone(), sd[key + '.bias'].clone()


def _check(y, E, S, bound, what):
    d = (y - E).abs()
    bad = d > bound
    print(f'{what}: max |y - E| {d.max().item():.3e}, largest share of its bound {(d / bound).max().item():.3f}')
    assert not bool(bad.any()), (what, int(bad.sum()), (d / bound).max().item())


SHAPES = [(134, 320), (144, 180), (37, 53), (3, 3)]


# ---- 1. per layer, derived bound ------------------------------------------------------------------------------

def test_weight_packers_match_the_host_statement(ops):
    for transposed, cin, cout in ((False, 64, 64), (False, 51, 64), (False, 15, 64), (True, 64, 64)):
        w = torch.randn((cin, cout, 3, 3) if transposed else (cout, cin, 3, 3), generator=_gen(5)) * 0.1
        got = ops.f16_pack_weights(w.cuda().contiguous(), transposed).cpu().numpy()
        idx = ops.f16_pack_index(transposed, cin, cout)
        exp = np.where(idx >= 0, w.reshape(-1).numpy()[np.maximum(idx, 0)], 0).astype(np.float16)   # numpy rounds to nearest even
        assert np.array_equal(got.view(np.uint16), exp.view(np.uint16)), (transposed, cin, cout)


@pytest.mark.parametrize('h,w', SHAPES)
@pytest.mark.parametrize('n', [1, 3])
def test_pack_input_is_the_rounded_concatenation(ops, n, h, w):
    for c2 in (48, 12):
        x1 = torch.randn(n, 3, h, w, generator=_gen(1)) * 0.7
        x2 = torch.randn(n, c2, h, w, generator=_gen(2)) * 300.0
        got = ops.f16_pack_input(x1.cuda(), x2.cuda()).cpu()
        exp = torch.zeros(n, h, w, 64, dtype=torch.float16)
        exp[..., :3 + c2] = torch.cat([x1, x2], 1).permute(0, 2, 3, 1).to(torch.float16)           # torch rounds to nearest even
        assert torch.equal(got.view(torch.int16), exp.view(torch.int16)), (n, h, w, c2)


@pytest.mark.parametrize('h,w', SHAPES)
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('amp', [1.0, 1000.0])
def test_conv3x3_f16_within_the_derived_bound(ops, n, h, w, amp):
    """ReLU on / off x skip on / off, activations at the procedural network's scale and up to 1000."""
    _, wt, b = _body_weights()
    wt = _h(wt)
    if amp > 1:
        wt = _h(wt * 0.5)
    x = _h((torch.rand(n, 64, h, w, generator=_gen(11)) * 2 - 1) * amp)
    res = _h((torch.rand(n, 64, h, w, generator=_gen(12)) * 2 - 1) * amp)
    wp = ops.f16_pack_weights(wt.cuda().contiguous())
    xg, rg, bg = _nhwc16(x), _nhwc16(res), b.cuda()
    for relu in (False, True):
        for skip in (False, True):
            E, S = FX.layer_ref(x, wt, b, relu, res if skip else None)
            assert E.abs().max().item() < FX.F16_MAX
            y = ops.conv3x3_f16(xg, wp, bg, act=ops.ACT_RELU if relu else ops.ACT_NONE, res=rg if skip else None)
            _check(_nchw(y), E, S, FX.bound_f16_out(E, S), f'conv3x3_f16 n={n} {h}x{w} amp={amp} relu={relu} skip={skip}')
    # in place over the skip input (what the plan does)
    E, S = FX.layer_ref(x, wt, b, False, res)
    buf = rg.clone()
    ops.conv3x3_f16(xg, wp, bg, act=ops.ACT_NONE, res=buf, out=buf)
    _check(_nchw(buf), E, S, FX.bound_f16_out(E, S), 'conv3x3_f16 in place')


@pytest.mark.parametrize('h,w', SHAPES)
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('scale,c2', [(4, 48), (2, 12)])
def test_conv_in_f16_within_the_derived_bound(ops, n, h, w, scale, c2):
    """conv_in: two fp32 NCHW sources (3 + 48 channels at 4x, 3 + 12 at 2x), packed, K padded with zero weights."""
    sd = generator_state_dict(scale=scale, degradation='BD' if scale == 4 else 'BI')
    wt, b = _h(sd['srnet.conv_in.0.weight']), sd['srnet.conv_in.0.bias']
    assert wt.shape[1] == 3 + c2
    x1 = _h(torch.rand(n, 3, h, w, generator=_gen(21)))
    x2 = _h(torch.rand(n, c2, h, w, generator=_gen(22)))
    E, S = FX.layer_ref(torch.cat([x1, x2], 1), wt, b, True)
    y = ops.conv3x3_f16(ops.f16_pack_input(x1.cuda(), x2.cuda()), ops.f16_pack_weights(wt.cuda().contiguous()), b.cuda(),
                        act=ops.ACT_RELU)
    _check(_nchw(y), E, S, FX.bound_f16_out(E, S), f'conv_in {scale}x n={n} {h}x{w}')


@pytest.mark.parametrize('h,w', SHAPES)
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('amp', [1.0, 1000.0])
def test_convt3x3s2_f16_within_the_derived_bound(ops, n, h, w, amp):
    sd = generator_state_dict(scale=4, degradation='BD')
    wt, b = _h(sd['srnet.conv_up.0.weight']), sd['srnet.conv_up.0.bias']
    x = _h((torch.rand(n, 64, h, w, generator=_gen(31)) * 2 - 1) * amp)
    wp = ops.f16_pack_weights(wt.cuda().contiguous(), transposed=True)
    for relu in (False, True):
        E, S = FX.layer_ref(x, wt, b, relu, transposed=True)
        assert E.abs().max().item() < FX.F16_MAX
        y = torch.full((n, 64, 2 * h, 2 * w), 7.0, device='cuda')
        ops.convt3x3s2_f16(_nhwc16(x), wp, b.cuda(), act=ops.ACT_RELU if relu else ops.ACT_NONE, out=y)
        _check(y.cpu().double(), E, S, FX.bound_f32_out(E, S), f'convt3x3s2_f16 n={n} {h}x{w} amp={amp} relu={relu}')


def test_batch_equals_single_frames_bit_for_bit(ops):
    _, wt, b = _body_weights()
    wp = ops.f16_pack_weights(wt.cuda().contiguous())
    x = (torch.randn(3, 37, 53, 64, generator=_gen(41)) * 0.5).to(torch.float16).cuda()
    both = ops.conv3x3_f16(x, wp, b.cuda(), act=ops.ACT_RELU)
    for i in range(3):
        one = ops.conv3x3_f16(x[i:i + 1].contiguous(), wp, b.cuda(), act=ops.ACT_RELU)
        assert torch.equal(both[i:i + 1].view(torch.int16), one.view(torch.int16)), i


# ---- 2. whole SRNet body, teacher-forced -----------------------------------------------------------------------

@pytest.mark.parametrize('scale,deg,h,w', [(4, 'BD', 37, 53), (2, 'BI', 64, 96)])
def test_srnet_body_teacher_forced(ops, scale, deg, h, w):
    """One fp16 frame through the per-layer entry points with the procedural weights; every layer's output is checked
    against torch float64 on the kernel's OWN input for that layer (all 22 layers, no amplification)."""
    sd = FX.O._sub(generator_state_dict(scale=scale, degradation=deg), 'srnet.')
    keys, nb = FX.body_keys(sd)
    assert len(keys) == 22
    wts = {k: _h(sd[k + '.weight']) for k in keys}
    wps = {k: ops.f16_pack_weights(wts[k].cuda().contiguous(), transposed=(k == 'conv_up.0')) for k in keys}
    bs = {k: sd[k + '.bias'] for k in keys}
    lr_curr = smooth_clip(1, 3, h, w, seed=9)
    s2d = torch.rand(1, scale * scale * 3, h, w, generator=_gen(51))
    xin = ops.f16_pack_input(lr_curr.cuda(), s2d.cuda())
    exp_in = torch.cat([lr_curr, s2d], 1).to(torch.float16)
    assert torch.equal(xin.cpu()[..., :exp_in.shape[1]].permute(0, 3, 1, 2), exp_in) and not bool(xin[..., exp_in.shape[1]:].any())

    def layer(k, x16, relu, res16=None):
        cin = wts[k].shape[1]
        E, S = FX.layer_ref(_nchw(x16)[:, :cin].float(), wts[k], bs[k], relu, None if res16 is None else _nchw(res16).float())
        y = ops.conv3x3_f16(x16, wps[k], bs[k].cuda(), act=ops.ACT_RELU if relu else ops.ACT_NONE, res=res16)
        _check(_nchw(y), E, S, FX.bound_f16_out(E, S), f'{scale}x {k}')
        return y
    out = layer('conv_in.0', xin, True)
    for b in range(nb):
        t = layer(f'resblocks.{b}.conv.0', out, True)
        out = layer(f'resblocks.{b}.conv.2', t, False, out)
    E, S = FX.layer_ref(_nchw(out).float(), wts['conv_up.0'], bs['conv_up.0'], True, transposed=True)
    y = ops.convt3x3s2_f16(out, wps['conv_up.0'], bs['conv_up.0'].cuda(), act=ops.ACT_RELU)
    _check(y.cpu().double(), E, S, FX.bound_f32_out(E, S), f'{scale}x conv_up.0')


# ---- 3. whole clips against the reference-made golden ----------------------------------------------------------

def _net(scale, deg, precision='fp32'):
    from tecogan_pytorch_amd.models.networks import FRNet
    net = FRNet(3, 3, 64, 10, deg, scale, precision=precision)
    net.load_state_dict(generator_state_dict(scale=scale, degradation=deg), strict=True)
    return net.cuda().eval()


def _step_clip(net, clip, scale):
    """frame by frame through FRNet.step: float frames (t, c, H, W) and uint8 frames (t, H, W, c)"""
    t, c, h, w = clip.shape
    dev_clip = clip.cuda()
    lp = torch.zeros(1, c, h, w, device='cuda')
    hp = torch.zeros(1, c, scale * h, scale * w, device='cuda')
    fl, u8 = [], []
    with torch.no_grad():
        for i in range(t):
            q = torch.empty(1, scale * h, scale * w, c, dtype=torch.uint8, device='cuda')
            hc = net.step(dev_clip[i:i + 1], lp, hp, u8_out=q)
            lp, hp = dev_clip[i:i + 1], hc
            fl.append(hc[0].cpu().numpy()); u8.append(q[0].cpu().numpy())
    net.check_faults()
    return np.stack(fl), np.stack(u8)


@pytest.mark.parametrize('name', FX.CLIPS)
def test_whole_clip_against_the_reference_golden(name):
    """FRNet(precision='fp16') through the plan against `spec` (the reference network with the specification's rounding
    points and float64 accumulation): at most twice the distance of the reference's own fp32-accumulating run (`alt`)
    from `spec` -- the project's triangulation margin -- and never more than one uint8 level."""
    g = FX.load(name)
    s, deg = g['scale'], g['degradation']
    clip = smooth_clip(g['t'], 3, g['h'], g['w'], seed=g['seed'])
    net = _net(s, deg, 'fp16')
    fl, u8s = _step_clip(net, clip, s)
    runs = {'step': u8s,
            'infer_sequence': net.infer_sequence(clip, 'cuda', pipeline=False),
            'infer_sequence pipelined': net.infer_sequence(clip, 'cuda', pipeline=True),
            'infer_sequence device': net.infer_sequence(clip.cuda(), 'cuda', return_device_tensor=True).cpu().numpy()}
    torch.cuda.synchronize()
    net.check_faults()
    r0, r1 = FX.rel_l2(fl[0], g['hr_first']), FX.rel_l2(fl[-1], g['hr_last'])
    print(f'{name}: relL2(HIP, spec) first {r0:.3e} (noise {g["noise_rel_l2"][0]:.3e}), last {r1:.3e} (noise {g["noise_rel_l2"][-1]:.3e})')
    fails = []
    for tag, u8 in runs.items():
        assert u8.shape == g['u8'].shape, tag
        for i in range(g['t']):
            share, mx = FX.u8_diff(u8[i], g['u8'][i])
            print(f'{name} {tag} frame {i}: u8 share {share:.5f} (noise {g["noise_u8_share"][i]:.5f}), max {mx}')
            if share > 2 * g['noise_u8_share'][i] or mx > 1:
                fails.append((tag, i, share, mx))
    assert r0 <= 2 * g['noise_rel_l2'][0] and r1 <= 2 * g['noise_rel_l2'][-1], (r0, r1)
    assert not fails, fails


# ---- 4. plan = layers ------------------------------------------------------------------------------------------

def _kinds(plan):
    from tecogan_pytorch_amd import _lib as L
    lib = L.lib()
    out = {}
    for k in range(lib.tg_frnet_plan_kinds()):
        nl = ctypes.c_int()
        L.check(lib.tg_frnet_plan_kind_stats(plan.handle, k, ctypes.byref(nl), None, None), 'kind_stats')
        out[lib.tg_frnet_kind_name(k).decode()] = nl.value
    return out, lib.tg_frnet_plan_launches(plan.handle)


F16_KINDS = ('pack_input_f16_kernel', 'conv3x3_f16_kernel<false>', 'conv3x3_f16_kernel<true>')


@pytest.mark.parametrize('h,w', [(134, 320), (37, 53)])
@pytest.mark.parametrize('n', [1, 2])
def test_plan_frame_equals_the_layer_entry_points_bit_for_bit(ops, n, h, w):
    """tg_frnet_step_srnet of an fp16 plan = the warp entry point, the fp16 per-layer entry points and the HR-stage
    entry points in the same order (4x)."""
    from tecogan_pytorch_amd import _lib as L
    s, deg = 4, 'BD'
    net = _net(s, deg, 'fp16')
    g = _gen(61)
    lr_curr = torch.rand(n, 3, h, w, generator=g).cuda()
    hr_prev = torch.rand(n, 3, s * h, s * w, generator=g).cuda()
    lr_flow = ((torch.rand(n, 2, h // 8 * 8, w // 8 * 8, generator=g) - 0.5) * 3).cuda()
    plan = net._get_plan(n, h, w, torch.device('cuda', 0))
    assert plan.precision == 'fp16' and L.lib().tg_frnet_plan_precision(plan.handle) == L.PREC_F16
    out = torch.empty(n, 3, s * h, s * w, device='cuda')
    u8 = torch.empty(n, s * h, s * w, 3, dtype=torch.uint8, device='cuda')
    L.check(L.lib().tg_frnet_step_srnet(plan.handle, lr_flow.data_ptr(), lr_curr.data_ptr(), hr_prev.data_ptr(),
                                        out.data_ptr(), u8.data_ptr(), torch.cuda.current_stream().cuda_stream), 'step_srnet')
    faults, active = plan.chain_state()
    assert faults == 0 and not active                     # no workgroup of the fp16 body waits for another one
    sr = net.srnet
    body = sr.layers()[:22]
    s2d = ops.flowup_warp_s2d(lr_flow, hr_prev, h, w, s, sr.up_mode())
    x = ops.f16_pack_input(lr_curr, s2d)
    wp = [ops.f16_pack_weights(m.weight.detach().contiguous(), transposed=(i == 21)) for i, m in enumerate(body)]
    bs = [m.bias.detach().contiguous() for m in body]
    a = ops.conv3x3_f16(x, wp[0], bs[0], act=ops.ACT_RELU)
    for b in range(10):
        t = ops.conv3x3_f16(a, wp[1 + 2 * b], bs[1 + 2 * b], act=ops.ACT_RELU)
        a = ops.conv3x3_f16(t, wp[2 + 2 * b], bs[2 + 2 * b], act=ops.ACT_NONE, res=a, out=a)
    u1 = ops.convt3x3s2_f16(a, wp[21], bs[21], act=ops.ACT_RELU)
    up2, conv_out = sr.layers()[-2:]
    wa = ops.convt_pack_wino(up2.packed()[0], 64, 64)
    wz = ops.convt_pack_wz(conv_out.weight.detach().contiguous())
    z = ops.convt3x3s2_z_wino(u1, wa, up2.bias.detach().contiguous(), wz, 3, 64, act=ops.ACT_RELU)
    hr, q = ops.convout_tail(z, 3, conv_out.bias.detach().contiguous(), up_src=lr_curr, up_mode=sr.up_mode(), up_scale=s,
                             want_u8=True)
    torch.cuda.synchronize()
    assert torch.equal(hr, out), (hr - out).abs().max().item()
    assert torch.equal(q, u8)


def test_switching_to_fp16_and_back_is_bit_identical_to_never_leaving_fp32():
    s, deg, h, w = 4, 'BD', 134, 320
    clip = smooth_clip(4, 3, h, w, seed=71)
    ref = _net(s, deg).infer_sequence(clip, 'cuda')
    net = _net(s, deg)
    net.precision = 'fp16'
    half = net.infer_sequence(clip, 'cuda')
    net.precision = 'fp32'
    back = net.infer_sequence(clip, 'cuda')
    assert np.array_equal(back, ref)
    assert not np.array_equal(half, ref)                  # (the mode does something)
    share, mx = FX.u8_diff(half, ref)
    print(f'fp16 vs fp32 at {h}x{w}: u8 share {share:.5f}, max {mx}')
    assert mx <= 1
    # the plan-level switch on ONE plan, too
    from tecogan_pytorch_amd import _lib as L
    n32 = _net(s, deg)
    lr, lp = clip[1:2].cuda(), clip[0:1].cuda()
    hp = torch.rand(1, 3, s * h, s * w, generator=_gen(72)).cuda()
    with torch.no_grad():
        a = n32.step(lr, lp, hp).clone()
        plan = n32._get_plan(1, h, w, torch.device('cuda', 0))
        k32 = _kinds(plan)
        n16 = _net(s, deg, 'fp16')
        p16 = n16._get_plan(1, h, w, torch.device('cuda', 0))
        b16 = n16.step(lr, lp, hp).clone()
        L.check(L.lib().tg_frnet_plan_set_precision(p16.handle, L.PREC_F32, None, 0, None), 'set_precision')
        assert _kinds(p16) == k32
        c = n16.step(lr, lp, hp).clone()
    torch.cuda.synchronize()
    assert torch.equal(a, c) and not torch.equal(a, b16)


@pytest.mark.parametrize('name', FX.CLIPS)
def test_pipelined_and_frame_by_frame_agree_within_the_noise(name):
    """The batched flow pass picks other kernel forms than the per-frame one (existing tests allow one level on 0.2 %
    of the pixels in fp32); in fp16 mode a last-bit change of the flow flips roundings like any other: one level on at
    most twice the golden's noise share, nothing tighter."""
    g = FX.load(name)
    s, deg = g['scale'], g['degradation']
    clip = smooth_clip(g['t'], 3, g['h'], g['w'], seed=g['seed'])
    net = _net(s, deg, 'fp16')
    a = net.infer_sequence(clip, 'cuda', pipeline=True)
    b = net.infer_sequence(clip, 'cuda', pipeline=False)
    for i in range(g['t']):
        share, mx = FX.u8_diff(a[i], b[i])
        print(f'{name} frame {i}: pipelined vs frame by frame u8 share {share:.5f}, max {mx}')
        assert share <= 2 * g['noise_u8_share'][i] and mx <= 1, (i, share, mx)


# ---- 5. nothing leaks ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('scale,deg,h,w', [(4, 'BD', 134, 320), (4, 'BD', 37, 53), (2, 'BI', 64, 96)])
def test_fp32_plans_are_untouched_and_fp16_differs_in_the_body_only(scale, deg, h, w):
    from tecogan_pytorch_amd.models.networks import FRNet
    dflt = FRNet(3, 3, 64, 10, deg, scale)
    dflt.load_state_dict(generator_state_dict(scale=scale, degradation=deg), strict=True)
    dflt = dflt.cuda().eval()
    expl, half = _net(scale, deg, 'fp32'), _net(scale, deg, 'fp16')
    dev = torch.device('cuda', 0)
    kd, ke, kh = (_kinds(n_._get_plan(1, h, w, dev)) for n_ in (dflt, expl, half))
    assert kd == ke
    assert all(kd[0][k] == 0 for k in F16_KINDS)
    assert kh[0]['pack_input_f16_kernel'] == 1 and kh[0]['conv3x3_f16_kernel<false>'] == 21 and kh[0]['conv3x3_f16_kernel<true>'] == 1
    fnet_warp = ('flowup_warp_s2d_kernel', 'maxpool2_kernel', 'upsample_kernel', 'conv3x3_small_kernel' if scale == 4 else None)
    for k in fnet_warp:
        if k:
            assert kh[0][k] == kd[0][k], k
    if scale == 4:
        # the HR stage behind the first up-sampling layer: the same launches
        for k in ('convt3x3s2_mfma_kernel<Z>', 'convout_tail_kernel', 'quantize_u8_hwc_kernel'):
            assert kh[0][k] == kd[0][k], k
        # and nothing of the fp32 body is left
        for k in ('conv3x3_wino_resident_kernel', 'conv3x3_wino_chain_kernel'):
            assert kh[0][k] == 0, k
    clip = smooth_clip(2, 3, h, w, seed=81)
    lr, lp = clip[1:2].cuda(), clip[0:1].cuda()
    hp = torch.rand(1, 3, scale * h, scale * w, generator=_gen(82)).cuda()
    with torch.no_grad():
        a, b, c = dflt.step(lr, lp, hp), expl.step(lr, lp, hp), half.step(lr, lp, hp)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert (a - c).abs().max().item() < 4e-3             # one uint8 level; the issue measured 5.5e-4 .. 1.1e-3


def test_u8_batch_at_2x_is_refused_not_computed_in_fp32():
    """At 2x the fp16 body ends in the unfused output conv, whose uint8 form takes one frame: n > 1 with a uint8 output
    is TG_E_ARG, never a silent fp32 frame."""
    from tecogan_pytorch_amd import _lib as L
    net = _net(2, 'BI', 'fp16')
    n, h, w = 2, 32, 48
    lr = torch.rand(n, 3, h, w).cuda()
    hp = torch.rand(n, 3, 2 * h, 2 * w).cuda()
    q = torch.empty(n, 2 * h, 2 * w, 3, dtype=torch.uint8, device='cuda')
    with torch.no_grad():
        out = net.step(lr, lr, hp)                        # float output: fine
        with pytest.raises(L.TecoganHipError):
            net.step(lr, lr, hp, u8_out=q)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


def test_training_after_fp16_inference_is_unchanged():
    """A training step (the tape; forward_sequence) never uses the mode: an FRVSR iteration on a generator built with
    precision='fp16' that has just run an fp16 inference gives the log dict of the same iteration on an fp32
    generator that never inferred."""
    from tecogan_pytorch_amd.models import define_model
    crop, t, nclip, s = 32, 4, 2, 4

    def opt(precision):
        gen = {'name': 'FRNet', 'in_nc': 3, 'out_nc': 3, 'nf': 64, 'nb': 10, 'load_path': None}
        if precision:
            gen['precision'] = precision
        return {'scale': s, 'dist': False, 'device': 'cuda', 'rank': 0, 'world_size': 1, 'is_train': True,
                'dataset': {'degradation': {'type': 'BD', 'sigma': 1.5}, 'train': {'crop_size': crop}},
                'model': {'name': 'FRVSR', 'generator': gen},
                'train': {'tempo_extent': t, 'ckpt_dir': '/tmp', 'generator': {'lr': 1e-4, 'betas': [0.9, 0.999]},
                          'pixel_crit': {'type': 'CB', 'weight': 1, 'reduction': 'mean'},
                          'warping_crit': {'type': 'CB', 'weight': 1, 'reduction': 'mean'}},
                'logger': {'decay': 0.99}}
    gt = torch.stack([smooth_clip(t, 3, crop + 8, crop + 8, seed=100 + i, shift=1.0) for i in range(nclip)])
    logs, outs = [], []
    for precision in (None, 'fp16'):
        m = define_model(opt(precision))
        m.net_G.load_state_dict(generator_state_dict(scale=s, degradation='BD'), strict=True)
        if precision:
            assert m.net_G.precision == 'fp16'
            m.net_G.eval()
            m.net_G.infer_sequence(smooth_clip(3, 3, 37, 53, seed=5), 'cuda')
            m.net_G.train()
        m.prepare_training_data({'gt': gt})
        m.train()
        logs.append({k: float(v) for k, v in m.log_dict.items()})
        with torch.no_grad():
            m2 = define_model(opt(precision))        # the unroll itself, on the initial weights: no atomic adds in it
            m2.net_G.load_state_dict(generator_state_dict(scale=s, degradation='BD'), strict=True)
            if precision:
                m2.net_G.eval()
                m2.net_G.infer_sequence(smooth_clip(3, 3, 37, 53, seed=5), 'cuda')
                m2.net_G.train()
            outs.append(m2.net_G.forward_sequence(m.lr_data)['hr_data'].clone())
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])             # the training frames are the fp32 frames, bit for bit
    # The losses are sums of at most 4096 per-block partials (tg_train.hip: grid_for) added with fp32 atomics in
    # run-to-run order: two runs of the SAME computation differ by at most 2 (B - 1) 2^-24 relative.
    tol = 2 * 4095 * 2.0 ** -24
    assert logs[0] and logs[0].keys() == logs[1].keys()
    for k in logs[0]:
        assert abs(logs[0][k] - logs[1][k]) <= tol * abs(logs[0][k]), (k, logs)
