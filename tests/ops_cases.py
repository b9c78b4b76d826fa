"""One valid call of every public wrapper and class method of tecogan_pytorch_amd.ops that reaches ops._call: a plain
table for tests/test_ops_boundary_cpu.py and tests/test_hip_ops_boundary.py.

A row is (label, build, entry_names, host_operands): build(ops, device) -> (callable, kwargs) makes the smallest
arguments the wrapper's own shape checks admit (n <= 2, 8 x 8 maps, 16 x 16 where the flow pyramid needs them, two
segments per list, 64 channels only where the wrapper hard-wires them); entry_names is the set of tg_* names the call
may reach; host_operands names the keyword arguments that are host memory by design.  Every optional tensor operand is
given in some row, so that the tests can replace each in turn.  Nothing here launches a kernel: the tests keep a
recorder in the place of ops._call."""
import numpy as np
import torch

ROWS = []


def row(label, *entry_names, host=()):
    def add(build):
        ROWS.append((label, build, frozenset(entry_names), tuple(host)))
        return build
    return add


class T:
    """Tensor makers on one device."""

    def __init__(self, device):
        self.device = device

    def f(self, *shape):
        return torch.zeros(*shape, device=self.device)

    def h(self, *shape):
        return torch.zeros(*shape, dtype=torch.float16, device=self.device)

    def u8(self, *shape):
        return torch.zeros(*shape, dtype=torch.uint8, device=self.device)

    def u16(self, *shape):
        return torch.zeros(*shape, dtype=torch.int16, device=self.device).view(torch.uint16)

    def i64(self, *shape):
        return torch.zeros(*shape, dtype=torch.int64, device=self.device)


def simple(label, *entry_names, host=(), **static):
    """A row whose callable is ops.<first word of the label> and whose kwargs are `make`(T) plus the static ones."""
    def add(make):
        name = label.split('/')[0]
        row(label, *entry_names, host=host)(lambda ops, dev: (getattr(ops, name), dict(make(T(dev)), **static)))
        return make
    return add


# ---- conv3x3 and its packs -------------------------------------------------------------------------------------------
simple('pack_conv3x3', 'tg_conv3x3_pack')(lambda t: dict(weight=t.f(4, 3, 3, 3)))
simple('pack_conv3x3_dgrad', 'tg_conv3x3_pack')(lambda t: dict(weight=t.f(4, 3, 3, 3)))
simple('pack_conv3x3_m16', 'tg_conv3x3_pack16')(lambda t: dict(weight=t.f(4, 4, 3, 3)))
simple('conv3x3', 'tg_conv3x3_fwd', cin=3, cout=4, ocb=32, ksplit=1)(
    lambda t: dict(x=t.f(1, 2, 8, 8), wpk=t.f(16), bias=t.f(4), x2=t.f(1, 1, 8, 8), out=t.f(1, 4, 8, 8)))
simple('conv3x3/res_mask', 'tg_conv3x3_fwd_masked', cin=3, cout=4, ocb=32)(
    lambda t: dict(x=t.f(1, 3, 8, 8), wpk=t.f(16), bias=t.f(4), res=t.f(1, 4, 8, 8), relu_mask=t.f(1, 4, 8, 8)))
simple('conv3x3/splitk', 'tg_conv3x3_splitk_fwd', cin=3, cout=4, ocb=32, ksplit=2, pool=True)(
    lambda t: dict(x=t.f(1, 2, 8, 8), wpk=t.f(16), bias=t.f(4), x2=t.f(1, 1, 8, 8), out=t.f(1, 4, 4, 4)))
simple('conv3x3_phased', 'tg_conv3x3_fwd_phased_masked', cin=4, cout=4, ocb=32, tapsel=0, cphase=0, taps_phase0=0,
       taps_phase1=0)(
    lambda t: dict(x=t.f(1, 4, 8, 8), wpk=t.f(16), out=t.f(1, 4, 8, 8), relu_mask=t.f(1, 4, 8, 8)))
simple('conv3x3_phased/nomask', 'tg_conv3x3_fwd_phased_masked', 'tg_conv3x3_fwd_phased_splitk', cin=4, cout=4, ocb=32,
       tapsel=0, cphase=0, taps_phase0=0, taps_phase1=0)(lambda t: dict(x=t.f(1, 4, 8, 8), wpk=t.f(16)))
simple('chain_pack', 'tg_conv3x3_chain_pack', layout=64)(
    lambda t: dict(items=[(t.f(4, 4, 3, 3), 0, 4, 0), (t.f(4, 4, 3, 3), 0, 4, 2)]))
simple('conv3x3s2', 'tg_conv3x3s2_fwd', cin=4, cout=4)(
    lambda t: dict(x=t.f(1, 4, 8, 8), wpk=t.f(16), relu_mask=t.f(1, 4, 4, 4), out=t.f(1, 4, 4, 4)))
simple('convt3x3s2', 'tg_convt3x3s2_fwd', cout=4)(
    lambda t: dict(x=t.f(1, 4, 8, 8), wpk=t.f(16), bias=t.f(4), out=t.f(1, 4, 16, 16)))
simple('convt_pack_wz', 'tg_convt_pack_wz')(lambda t: dict(w_out_oihw=t.f(3, 4, 3, 3)))
simple('convt3x3s2_z', 'tg_convt3x3s2_z_fwd_form', cz=3, cout=4)(
    lambda t: dict(x=t.f(1, 4, 8, 8), wpk=t.f(16), bias=t.f(4), wz=t.f(2048), out=t.f(1, 32, 16, 16)))
simple('convt_pack_wino', 'tg_convt_pack_wino', cin=4, cout=4)(lambda t: dict(wpk=t.f(16)))
simple('convt3x3s2_z_wino', 'tg_convt3x3s2_z_wino_fwd', cz=3, cout=4)(
    lambda t: dict(x=t.f(1, 4, 8, 8), wa=t.f(16), bias=t.f(4), wz=t.f(2048), out=t.f(1, 32, 16, 16)))
simple('convout_tail', 'tg_convout_tail_form', cz=3, up_mode=1, up_scale=4, want_u8=True)(
    lambda t: dict(z=t.f(1, 32, 8, 8), bias=t.f(3), up_src=t.f(1, 3, 2, 2)))
simple('conv3x3_fewin', 'tg_conv3x3_fewin_fwd')(
    lambda t: dict(x=t.f(1, 3, 8, 8), w_oihw=t.f(4, 3, 3, 3), relu_mask=t.f(1, 4, 8, 8), out=t.f(1, 4, 8, 8)))
simple('conv3x3_small', 'tg_conv3x3_small_fwd', up_mode=1, up_scale=4)(
    lambda t: dict(x=t.f(1, 4, 8, 8), weight=t.f(3, 4, 3, 3), bias=t.f(3), up_src=t.f(1, 3, 2, 2), out=t.f(1, 3, 8, 8)))
simple('conv3x3_small/res', 'tg_conv3x3_small_fwd_res')(
    lambda t: dict(x=t.f(1, 4, 8, 8), weight=t.f(3, 4, 3, 3), bias=t.f(3), res=t.f(1, 3, 8, 8)))

# ---- warps, resampling, quantisation ---------------------------------------------------------------------------------
simple('flowup_warp_s2d', 'tg_flowup_warp_s2d_fwd', h=8, w=8, scale=4, up_mode=1, want_hr_flow=True)(
    lambda t: dict(lr_flow=t.f(1, 2, 8, 8), hr_prev=t.f(1, 3, 32, 32), out=t.f(1, 48, 8, 8)))
simple('backward_warp', 'tg_backward_warp_fwd')(lambda t: dict(x=t.f(1, 3, 8, 8), flow=t.f(1, 2, 8, 8)))
simple('backward_warp_s2d', 'tg_backward_warp_s2d_fwd', scale=2)(lambda t: dict(x=t.f(1, 3, 8, 8), flow=t.f(1, 2, 8, 8)))
simple('space_to_depth', 'tg_space_to_depth', scale=2)(lambda t: dict(x=t.f(1, 3, 8, 8)))
simple('upsample', 'tg_upsample_fwd', scale=2, up_mode=1)(lambda t: dict(x=t.f(1, 3, 8, 8)))
simple('maxpool2', 'tg_maxpool2_fwd')(lambda t: dict(x=t.f(1, 3, 8, 8)))
simple('quantize_u8_hwc', 'tg_quantize_u8_hwc')(lambda t: dict(x=t.f(3, 8, 8)))
simple('dequantize_u8_hwc', 'tg_dequantize_u8_hwc')(lambda t: dict(x=t.u8(1, 8, 8, 3)))

# ---- planar YUV, deinterlacing, PNG, scene cuts: an 8 x 8 4:2:0 frame has 96 samples -----------------------------------
simple('yuv420_to_rgb', 'tg_yuv420_to_rgb_f32', h=8, w=8)(lambda t: dict(yuv=t.u8(1, 96)))
simple('rgb_to_yuv420', 'tg_rgb_u8_to_yuv420')(lambda t: dict(rgb_hwc=t.u8(1, 8, 8, 3)))
simple('yuv420p_to_rgb', 'tg_yuv420p16_to_rgb_f32', h=8, w=8, depth=10)(
    lambda t: dict(yuv_u16=t.u16(1, 96), out=t.f(1, 3, 8, 8)))
simple('rgb_f32_to_yuv420p', 'tg_rgb_f32_to_yuv420p16', depth=10)(
    lambda t: dict(rgb_chw=t.f(1, 3, 8, 8), out=t.u16(1, 96)))
simple('yuv_to_rgb', 'tg_yuv_planar_to_rgb_f32', h=8, w=8)(lambda t: dict(yuv=t.u8(1, 96), out=t.f(1, 3, 8, 8)))
simple('rgb_to_yuv', 'tg_rgb_u8_to_yuv_planar')(lambda t: dict(rgb_hwc=t.u8(1, 8, 8, 3)))
simple('rgb_f32_to_yuv', 'tg_rgb_f32_to_yuv_planar16')(lambda t: dict(rgb_chw=t.f(1, 3, 8, 8), out=t.u16(1, 96)))
simple('deinterlace', 'tg_deinterlace_planar', h=8, w=8)(
    lambda t: dict(frames=t.u8(1, 96), prev=t.u8(96), out=t.u8(2, 96)))
simple('png_encode', 'tg_png_encode_u8')(lambda t: dict(rgb_hwc=t.u8(1, 8, 8, 3)))
simple('png_encode/lz77', 'tg_png_encode_lz_u8', lz77=True)(lambda t: dict(rgb_hwc=t.u8(1, 8, 8, 3)))
simple('scene_cut_flags', 'tg_scene_cut_flags', mad=1.0, hist=1.0, forced=[1])(lambda t: dict(frames=t.f(2, 3, 8, 8)))

# ---- metrics ---------------------------------------------------------------------------------------------------------
simple('psnr_sse_u8', 'tg_psnr_sse_u8')(lambda t: dict(true_hwc=t.u8(1, 8, 8, 3), pred_hwc=t.u8(1, 8, 8, 3)))
simple('luma_u8', 'tg_luma_u8')(lambda t: dict(rgb=t.u8(4, 3)))
simple('lpips_conv', 'tg_lpips_conv_fwd', cout=4, ks=3, stride=1, pad=1)(
    lambda t: dict(x0=t.f(1, 3, 8, 8), wt=t.f(27, 4), bias=t.f(4), x1=t.f(1, 3, 8, 8), out=t.f(2, 4, 8, 8)))
simple('lpips_conv/lut', 'tg_lpips_conv_fwd', cout=4, ks=3, stride=1, pad=1)(
    lambda t: dict(x0=t.u8(1, 8, 8, 3), wt=t.f(27, 4), bias=t.f(4), x1=t.u8(1, 8, 8, 3), lut=t.f(256, 3)))
simple('maxpool3s2', 'tg_maxpool3s2_fwd')(lambda t: dict(x=t.f(1, 2, 8, 8), out=t.f(1, 2, 3, 3)))
simple('lpips_head', 'tg_lpips_head', layer=4)(
    lambda t: dict(feat_true=t.f(2, 4, 8, 8), feat_pred=t.f(2, 4, 8, 8), lin=t.f(4), res=t.f(2, 5), total=t.f(2)))
simple('ssim_y_u8', 'tg_ssim_y_u8')(lambda t: dict(true_hwc=t.u8(1, 8, 8, 3), pred_hwc=t.u8(1, 8, 8, 3)))
simple('psnr_yfloat_sse_u8', 'tg_psnr_yfloat_sse_u8')(lambda t: dict(true_hwc=t.u8(1, 8, 8, 3), pred_hwc=t.u8(1, 8, 8, 3)))
simple('farneback_flow', 'tg_farneback_flow_u8')(lambda t: dict(frames_u8=t.u8(2, 16, 16, 3)))
simple('flow_epe_mean', 'tg_flow_epe_mean')(lambda t: dict(flow_a=t.f(1, 8, 8, 2), flow_b=t.f(1, 8, 8, 2)))
simple('tof', 'tg_farneback_flow_u8', 'tg_flow_epe_mean')(
    lambda t: dict(true_hwc=t.u8(2, 16, 16, 3), pred_hwc=t.u8(2, 16, 16, 3)))

# ---- training side: weight and bias gradients --------------------------------------------------------------------------
simple('wgrad3x3', 'tg_wgrad3x3')(lambda t: dict(p=t.f(1, 4, 8, 8), q=t.f(1, 3, 8, 8), grad=t.f(4, 3, 3, 3)))
simple('wgrad3x3/bias', 'tg_wgrad3x3_multi_bias')(
    lambda t: dict(p=t.f(1, 4, 8, 8), q=t.f(1, 3, 8, 8), grad=t.f(4, 3, 3, 3), bias_grad=t.f(4)))
simple('wgrad3x3_multi', 'tg_wgrad3x3_multi')(
    lambda t: dict(p_list=[t.f(1, 4, 8, 8), t.f(1, 4, 8, 8)], q_list=[t.f(1, 3, 8, 8), t.f(1, 3, 8, 8)],
                   grad=t.f(4, 3, 3, 3)))
simple('wgrad3x3_multi/bias', 'tg_wgrad3x3_multi_bias')(
    lambda t: dict(p_list=[t.f(1, 4, 8, 8), t.f(1, 4, 8, 8)], q_list=[t.f(1, 3, 8, 8), t.f(1, 3, 8, 8)],
                   grad=t.f(4, 3, 3, 3), bias_grad=t.f(4)))
simple('wgrad3x3_multi/phased', 'tg_wgrad3x3_multi_phased', phased=(0, 0, 0))(
    lambda t: dict(p_list=[t.f(1, 4, 8, 8), t.f(1, 4, 8, 8)], q_list=[t.f(1, 3, 8, 8), t.f(1, 3, 8, 8)],
                   grad=t.f(4, 3, 3, 3)))
simple('wgrad3x3_convt_multi', 'tg_wgrad3x3_convt_multi')(
    lambda t: dict(x_list=[t.f(1, 4, 4, 4), t.f(1, 4, 4, 4)], dz_list=[t.f(1, 3, 8, 8), t.f(1, 3, 8, 8)],
                   grad=t.f(4, 3, 3, 3), bias_grad=t.f(3)))
simple('wgrad3x3_body', 'tg_wgrad3x3_body')(
    lambda t: dict(dz_list=[t.f(3, 1, 4, 8, 8), t.f(3, 1, 4, 8, 8)], acts_list=[t.f(3, 1, 4, 8, 8), t.f(3, 1, 4, 8, 8)],
                   grads=[t.f(4, 4, 3, 3), t.f(4, 4, 3, 3)]))
simple('wgrad3x3_body/bias', 'tg_wgrad3x3_body_bias')(
    lambda t: dict(dz_list=[t.f(3, 1, 4, 8, 8), t.f(3, 1, 4, 8, 8)], acts_list=[t.f(3, 1, 4, 8, 8), t.f(3, 1, 4, 8, 8)],
                   grads=[t.f(4, 4, 3, 3), t.f(4, 4, 3, 3)], dbs=[t.f(4), t.f(4)]))
simple('bias_grad_body', 'tg_bias_grad_body')(
    lambda t: dict(dz_list=[t.f(3, 1, 4, 8, 8), t.f(3, 1, 4, 8, 8)], dbs=[t.f(4), t.f(4), t.f(4)]))
simple('bias_grad_multi', 'tg_bias_grad_multi')(lambda t: dict(dy_list=[t.f(1, 4, 8, 8), t.f(1, 4, 8, 8)], db=t.f(4)))
simple('bias_grad', 'tg_bias_grad')(lambda t: dict(dy=t.f(1, 4, 8, 8), db=t.f(4)))

# ---- training side: backward kernels -----------------------------------------------------------------------------------
simple('act_bwd', 'tg_act_bwd', act=1)(lambda t: dict(dy=t.f(1, 4, 8, 8), y=t.f(1, 4, 8, 8), out=t.f(1, 4, 8, 8)))
simple('maxpool2_bwd', 'tg_maxpool2_bwd')(lambda t: dict(x=t.f(1, 2, 8, 8), dy=t.f(1, 2, 4, 4)))
simple('upsample_bwd', 'tg_upsample_bwd', scale=2, up_mode=1)(lambda t: dict(dy=t.f(1, 2, 8, 8)))
simple('backward_warp_bwd', 'tg_backward_warp_bwd')(
    lambda t: dict(x=t.f(1, 3, 8, 8), flow=t.f(1, 2, 8, 8), dy=t.f(1, 3, 8, 8), dflow_out=t.f(1, 2, 8, 8)))
simple('backward_warp_bwd/acc', 'tg_backward_warp_bwd_acc')(
    lambda t: dict(x=t.f(1, 3, 8, 8), flow=t.f(1, 2, 8, 8), dy=t.f(1, 3, 8, 8), dflow_out=t.f(1, 2, 8, 8),
                   dimg_acc=t.f(1, 3, 8, 8)))
simple('backward_warp_bwd/s2d', 'tg_backward_warp_s2d_bwd', s2d=2)(
    lambda t: dict(x=t.f(1, 3, 8, 8), flow=t.f(1, 2, 8, 8), dy=t.f(1, 12, 4, 4), dflow_out=t.f(1, 2, 8, 8),
                   dimg_acc=t.f(1, 3, 8, 8)))
simple('depth_to_space', 'tg_depth_to_space', scale=2)(lambda t: dict(x=t.f(1, 8, 8, 8)))
simple('depth_to_space/act', 'tg_depth_to_space', 'tg_depth_to_space_act_bwd', scale=2, act=1)(
    lambda t: dict(x=t.f(1, 8, 8, 8), act_y=t.f(1, 2, 16, 16)))
simple('pack_conv4x4s2', 'tg_conv4x4s2_pack')(lambda t: dict(w=t.f(4, 4, 4, 4)))
simple('conv4x4s2', 'tg_conv4x4s2_fwd', co=4)(lambda t: dict(x=t.f(1, 4, 8, 8), w_fwd=t.f(256), out=t.f(1, 4, 4, 4)))
simple('conv4x4s2_dgrad', 'tg_conv4x4s2_dgrad', ci=4, act=1)(
    lambda t: dict(g=t.f(1, 4, 4, 4), w_dgrad=t.f(256), act_y=t.f(1, 4, 8, 8)))

# ---- losses, optimiser, batch norm, the critic's head ------------------------------------------------------------------
simple('charbonnier', 'tg_charbonnier', loss_scale=1.0, grad_scale=1.0)(
    lambda t: dict(x=t.f(1, 3, 8, 8), y=t.f(1, 3, 8, 8), loss_accum=t.f(1)))
simple('pixel_loss', 'tg_pixel_loss', mode=0, loss_scale=1.0, grad_scale=1.0)(
    lambda t: dict(x=t.f(1, 3, 8, 8), y=t.f(1, 3, 8, 8), loss_accum=t.f(1)))
simple('cosine_loss', 'tg_cosine_loss', loss_scale=1.0, grad_scale=1.0)(
    lambda t: dict(a=t.f(1, 4, 8, 8), b=t.f(1, 4, 8, 8), loss_accum=t.f(1)))
simple('channel_norm', 'tg_channel_norm')(lambda t: dict(x=t.f(1, 3, 8, 8), mean=t.f(3), std=t.f(3)))
simple('bce_logits', 'tg_bce_logits', target=1.0, scale=1.0, grad_scale=1.0)(
    lambda t: dict(x=t.f(2, 1), stats3=t.f(3), dx_out=t.f(2, 1)))
simple('bce_logits/lsgan', 'tg_lsgan_loss', target=1.0, scale=1.0, grad_scale=1.0, lsgan=True)(
    lambda t: dict(x=t.f(2, 1), stats3=t.f(3), dx_out=t.f(2, 1)))
simple('adam_step', 'tg_adam_step', lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1)(
    lambda t: dict(p=t.f(8), g=t.f(8), m=t.f(8), v=t.f(8)))
simple('adam_step/guarded', 'tg_adam_step_guarded', lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1)(
    lambda t: dict(p=t.f(8), g=t.f(8), m=t.f(8), v=t.f(8), skip=t.f(1)))
simple('axpy_', 'tg_axpy')(lambda t: dict(y=t.f(8), x=t.f(8)))
simple('div_scalar_', 'tg_div_scalar', d=2.0)(lambda t: dict(y=t.f(8), x=t.f(8)))
simple('bn_lrelu_train_fwd', 'tg_bn_lrelu_train_fwd')(
    lambda t: dict(x=t.f(2, 4, 8, 8), gamma=t.f(4), beta=t.f(4), running_mean=t.f(4), running_var=t.f(4),
                   out=t.f(2, 4, 8, 8)))
simple('bn_lrelu_train_bwd', 'tg_bn_lrelu_train_bwd')(
    lambda t: dict(x=t.f(2, 4, 8, 8), y=t.f(2, 4, 8, 8), dy=t.f(2, 4, 8, 8), gamma=t.f(4), mean=t.f(4), invstd=t.f(4),
                   dgamma=t.f(4), dbeta=t.f(4), dx_out=t.f(2, 4, 8, 8)))
simple('linear1_fwd', 'tg_linear1_fwd')(lambda t: dict(x=t.f(2, 4), w=t.f(4), b=t.f(1)))
simple('linear1_bwd', 'tg_linear1_bwd')(lambda t: dict(x=t.f(2, 4), w=t.f(4), dy=t.f(2, 1), dw=t.f(4), db=t.f(1)))
_SYNC_FWD = ('tg_bn_local_stats', 'tg_bn_merge_stats', 'tg_bn_lrelu_apply')
_SYNC_BWD = ('tg_bn_lrelu_bwd_reduce', 'tg_axpy', 'tg_bn_lrelu_bwd_apply')
simple('sync_bn_lrelu_train_fwd_groups', *_SYNC_FWD, groups=2)(
    lambda t: dict(x=t.f(2, 4, 8, 8), gamma=t.f(4), beta=t.f(4), running_mean=t.f(4), running_var=t.f(4)))
simple('sync_bn_lrelu_train_fwd', *_SYNC_FWD)(
    lambda t: dict(x=t.f(2, 4, 8, 8), gamma=t.f(4), beta=t.f(4), running_mean=t.f(4), running_var=t.f(4)))
simple('sync_bn_lrelu_train_bwd_groups', *_SYNC_BWD, groups=2)(
    lambda t: dict(x=t.f(2, 4, 8, 8), y=t.f(2, 4, 8, 8), dy=t.f(2, 4, 8, 8), gamma=t.f(4),
                   stats=[(t.f(4), t.f(4), 64.0), (t.f(4), t.f(4), 64.0)], dgamma=t.f(4), dbeta=t.f(4)))
simple('sync_bn_lrelu_train_bwd', *_SYNC_BWD, count=128.0)(
    lambda t: dict(x=t.f(2, 4, 8, 8), y=t.f(2, 4, 8, 8), dy=t.f(2, 4, 8, 8), gamma=t.f(4), mean=t.f(4), invstd=t.f(4),
                   dgamma=t.f(4), dbeta=t.f(4)))


@row('fault_to_slot', 'tg_fault_to_slot', host=('err_pinned',))
def _fault_to_slot(ops, dev):
    err = torch.zeros(16, dtype=torch.int32)        # train_chain.py's pinned counter; unpinned where there is no device
    return ops.fault_to_slot, dict(err_pinned=err.pin_memory() if torch.device(dev).type == 'cuda' else err,
                                   slot=T(dev).f(1))


# ---- degradations and resizing -----------------------------------------------------------------------------------------
simple('downsample_bd', 'tg_downsample_bd', kernel2d=np.full((3, 3), 1 / 9, dtype=np.float32), scale=2, pad=True)(
    lambda t: dict(x=t.f(1, 3, 8, 8)))
simple('downsample_bi', 'tg_downsample_bi_u8', scale=2, out='both')(lambda t: dict(x=t.u8(1, 8, 8, 3)))
simple('downsample_bi/f32', 'tg_downsample_bi_f32', scale=2)(lambda t: dict(x=t.f(1, 3, 8, 8)))
simple('resize_u8', 'tg_resample_u8', size=(4, 4))(lambda t: dict(x=t.u8(1, 8, 8, 3), out=t.u8(1, 4, 4, 3)))

# ---- data movement of the training step --------------------------------------------------------------------------------
simple('time_gather', 'tg_time_gather', idx=[0, 2])(lambda t: dict(x=t.f(1, 3, 2, 8, 8)))
simple('pingpong', 'tg_time_gather')(lambda t: dict(x=t.f(1, 3, 2, 8, 8)))
simple('pingpong_grad', 'tg_pingpong_grad', te=3)(lambda t: dict(g=t.f(1, 2, 2, 8, 8)))
simple('d_assemble_fwd', 'tg_d_assemble_fwd', t=3, pad=0, crop=0)(
    lambda t: dict(data=t.f(1, 3, 3, 8, 8), warped=t.f(3, 3, 8, 8), cond=t.f(1, 3, 3, 8, 8), out=t.f(1, 27, 8, 8)))
simple('d_assemble_bwd', 'tg_d_assemble_bwd', n=1, t=3, t_data=3, c=3, pad=0, crop=0)(lambda t: dict(g=t.f(1, 27, 8, 8)))
simple('transpose01', 'tg_transpose01')(lambda t: dict(x=t.f(2, 3, 4)))
simple('stack_time', 'tg_stack_time')(lambda t: dict(frames=[t.f(2, 4), t.f(2, 4)]))
simple('index_gather', 'tg_index_gather', accumulate=True)(lambda t: dict(src=t.f(8), idx=t.i64(4), out=t.f(4)))

# ---- Winograd, the up-sampling conv, the one-launch chains ---------------------------------------------------------------
simple('pack_conv3x3_wino', 'tg_pack_conv3x3_wino')(lambda t: dict(w=t.f(4, 4, 3, 3)))
simple('conv3x3_wino', 'tg_conv3x3_wino_fwd', cin=3, cout=4)(
    lambda t: dict(x=t.f(1, 2, 8, 8), u_packed=t.f(16), bias=t.f(4), x2=t.f(1, 1, 8, 8), res=t.f(1, 4, 8, 8),
                   mask=t.f(1, 4, 8, 8), out=t.f(1, 4, 8, 8)))
simple('conv3x3_wino/pool', 'tg_conv3x3_wino_fused_fwd', cin=4, cout=4, pool=True)(
    lambda t: dict(x=t.f(1, 4, 8, 8), u_packed=t.f(16), bias=t.f(4), out=t.f(1, 4, 4, 4)))
simple('pack_upconv', 'tg_upconv_pack')(lambda t: dict(w=t.f(32, 64, 3, 3)))
simple('upconv_tap_gemm', 'tg_upconv_tap_gemm', cin=4, cout=2)(
    lambda t: dict(x=t.f(1, 4, 8, 8), a_packed=t.f(72), z=t.f(1, 18, 8, 8)))
simple('upconv_combine', 'tg_upconv_combine', cout=2)(
    lambda t: dict(z=t.f(1, 18, 8, 8), bias=t.f(2), out=t.f(1, 2, 16, 16)))
simple('upconv3x3', 'tg_upconv3x3_fwd', cin=4, cout=2)(
    lambda t: dict(x=t.f(1, 4, 8, 8), a_packed=t.f(72), bias=t.f(2), out=t.f(1, 2, 16, 16)))


def _row_layers(t):
    y0 = t.f(1, 4, 8, 8)
    return [dict(x=t.f(1, 2, 8, 8), x2=t.f(1, 2, 8, 8), w=t.f(4, 4, 3, 3), bias=t.f(4), y=y0),
            dict(x=y0, w=t.f(4, 4, 3, 3), bias=t.f(4), res=t.f(1, 4, 8, 8), mask=t.f(1, 4, 8, 8), y=t.f(1, 4, 8, 8))]


def _wino_layers(t):
    y0 = t.f(1, 4, 8, 8)
    return [dict(x=t.f(1, 2, 8, 8), x2=t.f(1, 2, 8, 8), u=t.f(16), bias=t.f(4), cin=4, y=y0),
            dict(x=y0, u=t.f(16), bias=t.f(4), cin=4, res=t.f(1, 4, 8, 8), y=t.f(1, 4, 8, 8))]


_ROW_PACKS = ('tg_conv3x3_pack16', 'tg_conv3x3_pack')
row('RowChain', *_ROW_PACKS)(lambda ops, dev: (ops.RowChain, dict(layers=_row_layers(T(dev)), n=1, h=8, w=8)))
row('RowChain.run', *_ROW_PACKS, 'tg_conv3x3_chain')(
    lambda ops, dev: (lambda layers: ops.RowChain(layers, 1, 8, 8).run(), dict(layers=_row_layers(T(dev)))))
row('WinoChain.run', 'tg_conv3x3_wino_chain')(
    lambda ops, dev: (lambda layers: ops.WinoChain(layers, 1, 4, 8, 8).run(), dict(layers=_wino_layers(T(dev)))))
row('WinoResident.run', 'tg_conv3x3_wino_resident')(
    lambda ops, dev: (lambda layers: ops.WinoResident(layers, 4, 8, 8).run(), dict(layers=_wino_layers(T(dev)))))
row('WinoResident.run/convt', 'tg_conv3x3_wino_resident_ct')(
    lambda ops, dev: (lambda layers, convt: ops.WinoResident(layers, 4, 8, 8).run(convt),
                      dict(layers=_wino_layers(T(dev)),
                           convt=dict(u=T(dev).f(16), bias=T(dev).f(64), y=T(dev).f(64, 16, 16), act=1))))
simple('pack_wres_convt', 'tg_conv3x3_wino_resident_ct_pack')(lambda t: dict(w=t.f(64, 64, 3, 3)))

# ---- fp16 inference body: 64 channels, channels-last -------------------------------------------------------------------
simple('f16_pack_weights', 'tg_conv3x3_f16_pack_weights')(lambda t: dict(w=t.f(4, 4, 3, 3)))
simple('f16_pack_input', 'tg_conv3x3_f16_pack_input')(lambda t: dict(x1=t.f(1, 2, 8, 8), x2=t.f(1, 2, 8, 8)))
simple('conv3x3_f16', 'tg_conv3x3_f16_fwd')(
    lambda t: dict(x=t.h(1, 8, 8, 64), w_packed=t.h(16), bias=t.f(64), res=t.h(1, 8, 8, 64), out=t.h(1, 8, 8, 64)))
simple('convt3x3s2_f16', 'tg_convt3x3s2_f16_fwd')(
    lambda t: dict(x=t.h(1, 8, 8, 64), w_packed=t.h(16), bias=t.f(64), out=t.f(1, 64, 16, 16)))


# ---- what the two test files share -------------------------------------------------------------------------------------
class Stop(Exception):
    """Raised by the recorder after it has recorded a wrapper that reads results back on the host."""


STOP_AFTER = frozenset({'tg_png_encode_u8', 'tg_png_encode_lz_u8', 'tg_psnr_yfloat_sse_u8'})


def recorder(monkeypatch, ops):
    """ops._call replaced by a function that records the name and launches nothing; returns the list of names."""
    seen = []

    def fake(name, *args):
        seen.append(name)
        if name in STOP_AFTER:
            raise Stop(name)
    monkeypatch.setattr(ops, '_call', fake)
    return seen


def tensor_paths(obj, path=()):
    """Every tensor inside nested dicts / lists / tuples, as (path of keys and indices, tensor)."""
    if torch.is_tensor(obj):
        yield path, obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            yield from tensor_paths(v, path + (k,))
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from tensor_paths(v, path + (i,))


def replaced(obj, path, new):
    """A copy of the nested arguments with the tensor at `path` replaced; the containers along the path are rebuilt,
    everything else is shared."""
    if not path:
        return new
    if isinstance(obj, dict):
        return {k: replaced(v, path[1:], new) if k == path[0] else v for k, v in obj.items()}
    return type(obj)(replaced(v, path[1:], new) if i == path[0] else v for i, v in enumerate(obj))
