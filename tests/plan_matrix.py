"""The case table of the frame-plan matrix (tests/test_plan_matrix_cpu.py, tests/test_hip_plan_matrix.py): one case per
launch-list decision of the frame plan (`choose` and `Emit::conv`, csrc/tg_api.hip), each as small as the branch allows.
Importable without a GPU.

A case is (name, nf, nb, scale, degradation, n, h, w, precision, env, expect) plus `extra`:

  env     the forcing switches of the child process that runs the case: TG_CONV_WINO, TG_WINO_CHAIN, TG_WINO_RES (read
          once per process by the library) and TG_WINO_RES_CT (read by the Python mirror at plan creation).  {} is the
          default rule.
  expect  {kind name (tg_frnet_kind_name): launches}: the kinds the case exists to reach, zeros included where the point
          of the case is that a kind is NOT used.
  extra   body     'resident' | 'chain' | 'layers': whether chain_state() must report a one-launch body
          claims   what the default rule says about this shape, as (rule, args..., answer) tuples that
                   tests/test_plan_matrix_cpu.py evaluates with the exported host functions (see CLAIMS there)
          u8       also ask for the uint8 frame;  phases: also run the two-phase / step_srnet comparisons
          fnet_only  k: the case is the flow-only plan of k frame pairs, consumed by tg_frnet_step_srnet on the frame
                   plan of one frame of the same (nf, nb, scale, degradation, h, w); `body` is about the flow-only
                   plan's statistics, frame_body says whether chain_state() of that frame plan reports a one-launch body

Where the thresholds come from (all read from the code, none from a run):

  tg_conv3x3_prefers_wino    cout % 64 == 0: ceil(w/32) * ceil(h/2) * (cout/64) * n >= 160 workgroups of 2 x 32 pixels;
                             cout == 32: ceil(w/64) * ceil(h/2) * n >= 2048; cin >= 16 (32 for cout = 32); never else.
  chain_wanted               768 < n * ceil(h/2) * ceil(w/32) <= 3000.
  CHAIN_MAX_LAYERS           24 layers in a one-launch body: 1 + 2 nb at 4x (conv_in has 51 input channels and joins),
                             2 nb at 2x (conv_in has 15 < 16: the direct form, in front of the body).
  conv3x3_wino_resident_ok   n = 1, nf = 64, h and w even (and one 8 x 24 block per CU, which no case here exceeds).
  conv3x3_rows_per_wg        the four-row direct form from n * h * w >= 200000 pixels of a 64-channel-group layer.
  conv3x3_uses_wg_ksplit     ceil(w/32) * ceil(h/2) * ceil(cout/64) * n <= 128 and cin >= 48; the one-shot form of it for
                             cin, cout <= 64; tg_conv3x3_pick_ksplit > 1 puts a finalize launch behind the conv instead.
  Z split rules              n = 1 and at least one whole round of 512 workgroup slots with a remainder:
                             ceil(zw/32) * ceil(zh/2) strips in the Winograd domain (nf = 64), ceil(zw/32) * ceil(zh/4)
                             workgroups with the last round 25..95 % full in the direct form; (zh, zw) = s/2 * (h, w).
  uint8 from the tail        four pixels a thread where the HR width s w is a multiple of 4 (always at 4x; at 2x for
                             an even w), one otherwise; the quantise launch only behind the unfused output conv when
                             that cannot emit the bytes itself (s w % 4 != 0), and only the fp16 body at 2x ends in it.

64x160 is the smallest even frame with 160 Winograd workgroups (32 x 5): at n = 1 the resident body with its tail, at
n = 2 one Winograd launch per layer, at n = 5 (800 tiles) the chain.  62x160 has 155 workgroups, 63x160 an odd height
(and an odd map at every FNet level), 66x158 a width that is no multiple of 4, 8 or 32 (ragged tiles, the
reflect-padded flow; its HR width 632 still is one of 4: the one-pixel tail is a 2x matter, 9x15 and 21x37 below).

nb = 0 is left out: the oracle finds nb as 1 + the largest `resblocks.N` key of the state dict and cannot express a
body without blocks.  nf < 32 is left out: the table covers nf 64, 48 and 32, and no plan with nf < 32 has ever run
(`cfg_ok` admits it; DESIGN.md section 7m, item 2, says what is known about it from reading).
"""
from collections import namedtuple

Case = namedtuple('Case', 'name nf nb scale degradation n h w precision env expect extra')

# kind names, as tg_frnet_kind_name returns them
R2, R4, C32 = 'conv3x3_mfma_kernel<2,2,1>', 'conv3x3_mfma_kernel<4,1,2>', 'conv3x3_mfma_kernel<4,1,1>'
CONVT, SMALL, WARP = 'convt3x3s2_mfma_kernel', 'conv3x3_small_kernel', 'flowup_warp_s2d_kernel'
POOL, UPS, QUANT, FINAL = 'maxpool2_kernel', 'upsample_kernel', 'quantize_u8_hwc_kernel', 'splitk_finalize_kernel'
KS, Z, TAIL, ONESHOT = 'conv3x3_mfma_kernel<1,2,1,KS=2>', 'convt3x3s2_mfma_kernel<Z>', 'convout_tail_kernel', 'conv3x3_oneshot_kernel'
WINO, CHAIN, RES = 'conv3x3_wino_kernel', 'conv3x3_wino_chain_kernel', 'conv3x3_wino_resident_kernel'
F16_PACK, F16_CONV, F16_CONVT = 'pack_input_f16_kernel', 'conv3x3_f16_kernel<false>', 'conv3x3_f16_kernel<true>'

# every kind is reached by some case; a kind that could not be would be listed here with the reason
NOT_REACHED = {}

MAX_FRAME_PIXELS = 134 * 320
FRAME_TOL, FLOW_TOL = 1e-4, 2e-4          # the project's bounds, stated at the top of tests/test_hip_parity.py


def cdiv(a, b):
    return (a + b - 1) // b


def body_tiles(c):
    """What chain_wanted is asked with: 2 x 32 pixel tiles of one full-resolution layer, over the batch."""
    return c.n * cdiv(c.h, 2) * cdiv(c.w, 32)


def body_layers(c):
    """Layers of a one-launch body (Choices::nchain of csrc/tg_api.hip)."""
    return 1 + 2 * c.nb if c.scale == 4 else 2 * c.nb


def _c(name, nf, nb, scale, deg, n, h, w, expect, precision='fp32', env=None, **extra):
    extra.setdefault('body', 'layers')
    extra.setdefault('claims', ())
    return Case(name, nf, nb, scale, deg, n, h, w, precision, dict(env or {}), dict(expect), extra)


W1, C1, C0, R1 = {'TG_CONV_WINO': '1'}, {'TG_WINO_CHAIN': '1'}, {'TG_WINO_CHAIN': '0'}, {'TG_WINO_RES': '1'}

CASES = [
    # ---- 4xBD, nf 64, nb 10: the flagship configuration beside every threshold of the default rule -----------------
    _c('res_tail_64x160', 64, 10, 4, 'BD', 1, 64, 160, {RES: 1, CHAIN: 0, WINO: 0, CONVT: 0, Z: 2, TAIL: 1, POOL: 2, UPS: 3,
                                                          WARP: 1, SMALL: 1, C32: 3},
       body='resident', u8=True, phases=True,
       claims=[('wino', 1, 64, 64, 64, 160, 1), ('wino', 1, 51, 64, 64, 160, 1), ('wgs', 64, 160, 160),
               ('resident_shape', 1), ('layers_fit', 1), ('zsplit_wino', 1), ('w4', 1)]),
    _c('wino_layers_n2_64x160', 64, 10, 4, 'BD', 2, 64, 160, {RES: 0, CHAIN: 0, WINO: 21, CONVT: 1, Z: 1, TAIL: 1},
       u8=True, claims=[('wino', 2, 64, 64, 64, 160, 1), ('tiles', 0), ('resident_shape', 0), ('zsplit_wino', 0)]),
    _c('chain_n5_64x160', 64, 10, 4, 'BD', 5, 64, 160, {RES: 0, CHAIN: 1, WINO: 8, CONVT: 1, R2: 2, FINAL: 2, POOL: 1, ONESHOT: 0},
       body='chain', u8=True,
       claims=[('tiles', 1), ('tiles_n', 4, 0), ('wino', 5, 32, 64, 32, 80, 1), ('wino', 5, 64, 128, 16, 40, 1),
               ('wino', 5, 128, 256, 8, 20, 0), ('layers_fit', 1)]),
    _c('direct_62x160', 64, 10, 4, 'BD', 1, 62, 160, {RES: 0, CHAIN: 0, WINO: 0, R2: 29, CONVT: 1, Z: 2},
       claims=[('wino', 1, 64, 64, 62, 160, 0), ('wgs', 62, 160, 155), ('resident_shape', 1)]),
    _c('odd_63x160', 64, 10, 4, 'BD', 1, 63, 160, {RES: 0, CHAIN: 0, WINO: 21, CONVT: 1, Z: 2, POOL: 2, FINAL: 8},
       u8=True, claims=[('wino', 1, 64, 64, 63, 160, 1), ('wgs', 63, 160, 160), ('resident_shape', 0), ('tiles', 0)]),
    _c('res_66x158', 64, 10, 4, 'BD', 1, 66, 158, {RES: 1, CHAIN: 0, WINO: 0, CONVT: 0, TAIL: 1, QUANT: 0},
       body='resident', u8=True, claims=[('wino', 1, 64, 64, 66, 158, 1), ('resident_shape', 1), ('w4', 1)]),
    _c('min_8x8', 64, 10, 4, 'BD', 1, 8, 8, {ONESHOT: 23, FINAL: 8, R2: 8, C32: 3, WINO: 0, RES: 0, Z: 1},
       u8=True, claims=[('wino', 1, 64, 64, 8, 8, 0), ('ksplit', 1, 64, 64, 8, 8, 1), ('ksplit_gt1', 1, 128, 256, 1, 1, 1)]),
    _c('odd_n3_26x45', 64, 10, 4, 'BD', 3, 26, 45, {ONESHOT: 23, WINO: 0, CHAIN: 0, CONVT: 1, Z: 1, TAIL: 1},
       u8=True, claims=[('wino', 3, 64, 64, 26, 45, 0), ('w4', 1)]),
    # ---- the 24-layer limit of a one-launch body: nb 11 is the last that fits at 4x, nb 12 at 2x --------------------
    _c('res_nb11_64x160', 64, 11, 4, 'BD', 1, 64, 160, {RES: 1, WINO: 0, CONVT: 0}, body='resident',
       claims=[('layers', 23), ('layers_fit', 1), ('resident_shape', 1)]),
    _c('layers_nb12_64x160', 64, 12, 4, 'BD', 1, 64, 160, {RES: 0, CHAIN: 0, WINO: 25, CONVT: 1},
       claims=[('layers', 25), ('layers_fit', 0), ('resident_shape', 1)]),
    _c('res_nb12_2x_64x160', 64, 12, 2, 'BI', 1, 64, 160, {RES: 1, WINO: 0, R2: 9, CONVT: 0, Z: 1}, body='resident',
       claims=[('layers', 24), ('layers_fit', 1), ('wino', 1, 15, 64, 64, 160, 0)]),
    _c('res_nb1_64x160', 64, 1, 4, 'BD', 1, 64, 160, {RES: 1, WINO: 0, CONVT: 0}, body='resident',
       claims=[('layers', 3), ('layers_fit', 1)]),
    # ---- 2xBI: conv_in in front of the body, one transposed conv (the Z launch), no tail on the resident launch ----
    _c('res_2x_64x160', 64, 10, 2, 'BI', 1, 64, 160, {RES: 1, CHAIN: 0, WINO: 0, R2: 9, CONVT: 0, Z: 1, TAIL: 1},
       body='resident', u8=True, phases=True,
       claims=[('wino', 1, 15, 64, 64, 160, 0), ('wino', 1, 64, 64, 64, 160, 1), ('resident_shape', 1), ('zsplit_wino', 0)]),
    _c('wino_layers_n2_2x_64x160', 64, 10, 2, 'BI', 2, 64, 160, {RES: 0, CHAIN: 0, WINO: 20, R2: 9, CONVT: 0},
       u8=True, claims=[('tiles', 0), ('resident_shape', 0)]),
    _c('chain_n5_2x_64x160', 64, 2, 2, 'BI', 5, 64, 160, {RES: 0, CHAIN: 1, WINO: 8, R2: 3}, body='chain',
       claims=[('tiles', 1), ('layers', 4), ('layers_fit', 1)]),
    _c('min_2x_9x15', 64, 10, 2, 'BI', 1, 9, 15, {ONESHOT: 22, R2: 9, WINO: 0, Z: 1, CONVT: 0}, u8=True,
       claims=[('wino', 1, 64, 64, 9, 15, 0), ('w4', 0)]),
    # the chain's upper edge, and the four-row direct form of conv_in beside its 200000-pixel threshold (nb 1: the
    # reference stays quick at 8 frames)
    _c('chain_top_n7_160x160', 64, 1, 2, 'BI', 7, 160, 160, {CHAIN: 1, WINO: 10, R2: 1, R4: 0}, body='chain',
       claims=[('tiles', 1), ('tiles_n', 8, 0), ('layers', 2), ('rows4', 0)]),
    _c('rows4_n8_160x160', 64, 1, 2, 'BI', 8, 160, 160, {CHAIN: 0, WINO: 12, R2: 0, R4: 1, POOL: 1},
       claims=[('tiles', 0), ('rows4', 1), ('wino', 8, 15, 64, 160, 160, 0)]),
    # ---- 2xBD and 4xBI, and the in-workgroup K split (encoder3.0 at 25x66: 78 two-row workgroups, 64 -> 128) --------
    _c('res_ks_2xBD_100x264', 64, 1, 2, 'BD', 1, 100, 264, {RES: 1, KS: 1, WINO: 0, Z: 1}, body='resident', u8=True,
       claims=[('ksplit', 1, 64, 128, 25, 66, 1), ('wg_ksplit', 64, 128, 25, 66, 1), ('wino', 1, 64, 64, 100, 264, 1),
               ('resident_shape', 1)]),
    _c('small_2xBD_21x37', 64, 2, 2, 'BD', 1, 21, 37, {ONESHOT: 6, R2: 9, WINO: 0}, u8=True,
       claims=[('wino', 1, 64, 64, 21, 37, 0), ('w4', 0)]),
    _c('res_4xBI_64x160', 64, 2, 4, 'BI', 1, 64, 160, {RES: 1, WINO: 0, CONVT: 0, Z: 2}, body='resident', u8=True,
       claims=[('resident_shape', 1)]),
    _c('small_4xBI_22x40', 64, 2, 4, 'BI', 2, 22, 40, {ONESHOT: 7, CONVT: 1, WINO: 0}, u8=True,
       claims=[('wino', 2, 64, 64, 22, 40, 0)]),
    # ---- nf 48 and 32: the direct Z form, never a Winograd body under the default rule ------------------------------
    _c('nf48_zsplit_128x160', 48, 2, 4, 'BD', 1, 128, 160, {WINO: 0, RES: 0, CHAIN: 0, R2: 13, CONVT: 1, Z: 2},
       u8=True, claims=[('wino', 1, 48, 48, 128, 160, 0), ('zsplit_direct', 1)]),
    _c('nf48_21x37', 48, 2, 4, 'BD', 1, 21, 37, {WINO: 0, ONESHOT: 7, Z: 1, CONVT: 1},
       claims=[('wino', 1, 48, 48, 21, 37, 0), ('zsplit_direct', 0)]),
    _c('nf32_2x_64x160', 32, 2, 2, 'BD', 1, 64, 160, {WINO: 0, RES: 0, C32: 8, Z: 1}, u8=True,
       claims=[('wino', 1, 32, 32, 64, 160, 0), ('zsplit_direct', 0)]),
    _c('nf32_4xBI_24x40', 32, 2, 4, 'BI', 2, 24, 40, {WINO: 0, C32: 8, CONVT: 1, Z: 1},
       claims=[('wino', 2, 32, 32, 24, 40, 0)]),
    # ---- the flow-only plans of the batched flow pass, consumed frame by frame through tg_frnet_step_srnet ---------
    # (n, h, w here are the FRAME plan's; the flow-only plan has `fnet_only` frame pairs.  Its statistics are the dry
    # run of the whole launch list at that batch, so WINO and R2 below include SRNet's 1 + 2 nb = 3 or 5 layers.)
    _c('fnet1_64x160', 64, 1, 4, 'BD', 1, 64, 160, {WINO: 3, POOL: 2, UPS: 3, FINAL: 7}, fnet_only=1, frame_body='resident'),
    _c('fnet2_26x45', 64, 1, 4, 'BD', 1, 26, 45, {POOL: 2, UPS: 3, FINAL: 8}, fnet_only=2, frame_body='layers'),
    _c('fnet8_64x160', 64, 1, 4, 'BD', 1, 64, 160, {WINO: 11, POOL: 1, UPS: 3, FINAL: 2, R2: 2}, fnet_only=8, frame_body='resident',
       claims=[('wino', 8, 32, 64, 32, 80, 1), ('wino', 8, 128, 256, 8, 20, 0), ('wino', 8, 32, 32, 64, 160, 0)]),
    # ---- fp16 body: one case per scale, launch kinds only (numerics: tests/test_hip_fp16.py) ------------------------
    _c('f16_4x_22x40', 64, 2, 4, 'BD', 1, 22, 40, {F16_PACK: 1, F16_CONV: 5, F16_CONVT: 1, CONVT: 0, Z: 1, TAIL: 1, RES: 0},
       precision='fp16', u8=True),
    _c('f16_2x_22x37', 64, 2, 2, 'BI', 1, 22, 37, {F16_PACK: 1, F16_CONV: 5, F16_CONVT: 1, CONVT: 0, Z: 0, TAIL: 0, SMALL: 2, QUANT: 1},
       precision='fp16', u8=True),
    # ---- forcing switches: branches the default rule takes only at sizes no test should run ------------------------
    # TG_CONV_WINO=1: the Winograd form at every size -- pool and x2 up-sampling folded into FNet's convs where the map
    # is even, the 32-channel workgroup (FNet's full-resolution layers, an nf 32 body), the resident body on a small frame
    _c('w1_res_22x40', 64, 10, 4, 'BD', 1, 22, 40, {RES: 1, WINO: 12, C32: 1, POOL: 2, UPS: 0, CONVT: 0}, env=W1,
       body='resident', u8=True),
    _c('w1_odd_21x37', 64, 2, 4, 'BD', 1, 21, 37, {RES: 0, CHAIN: 0, WINO: 17, POOL: 2, UPS: 0, CONVT: 1}, env=W1, u8=True),
    _c('w1_nf32_24x40', 32, 2, 2, 'BD', 1, 24, 40, {WINO: 16, C32: 2, POOL: 0, UPS: 0, RES: 0, CHAIN: 0}, env=W1, u8=True),
    _c('w1_nf48_24x40', 48, 2, 4, 'BI', 1, 24, 40, {WINO: 12, ONESHOT: 5, C32: 1, POOL: 0, UPS: 0}, env=W1),
    _c('w1_fnet8_22x40', 64, 2, 4, 'BD', 1, 22, 40, {WINO: 17, POOL: 2, UPS: 0}, env=W1, fnet_only=8, frame_body='resident'),
    # + TG_WINO_CHAIN=1: the chain at a small size, at n = 2 and (odd height: no resident body) at n = 1
    _c('w1c1_chain_n2_26x40', 64, 2, 4, 'BD', 2, 26, 40, {CHAIN: 1, RES: 0, WINO: 12, CONVT: 1, POOL: 1},
       env=dict(W1, **C1), body='chain', u8=True),
    _c('w1c1_chain_odd_21x37', 64, 2, 2, 'BI', 1, 21, 37, {CHAIN: 1, RES: 0, WINO: 12, R2: 1},
       env=dict(W1, **C1), body='chain', u8=True),
    # (nf 32 chains as well when both are forced: the chain runs the 64-channel workgroup with cout = 32.  The default
    # rule reaches this only with w <= 32 and 2048..3000 tile rows, 128 clips of 32x32 for one.)
    _c('w1c1_chain_nf32_24x40', 32, 2, 2, 'BD', 1, 24, 40, {CHAIN: 1, RES: 0, WINO: 12, C32: 2},
       env=dict(W1, **C1), body='chain', u8=True),
    # TG_WINO_RES=1 alone: the resident body where conv_in prefers the direct form and stays in front of it, at 4x
    # (the first transposed conv still rides on the launch: ct_fold does not ask where conv_in ran)
    _c('r1_res_convin_front_22x40', 64, 2, 4, 'BI', 1, 22, 40, {RES: 1, WINO: 0, ONESHOT: 3, CONVT: 0}, env=R1,
       body='resident', u8=True),
    # TG_WINO_RES=0 / TG_WINO_RES_CT=0 / TG_WINO_CHAIN=0 / TG_CONV_WINO=0: the other side of each default at the same frame
    _c('r0_layers_64x160', 64, 2, 4, 'BD', 1, 64, 160, {RES: 0, CHAIN: 0, WINO: 5, CONVT: 1, Z: 2}, env={'TG_WINO_RES': '0'}),
    _c('ct0_res_64x160', 64, 2, 4, 'BD', 1, 64, 160, {RES: 1, WINO: 0, CONVT: 1, Z: 2}, env={'TG_WINO_RES_CT': '0'},
       body='resident', phases=True),
    _c('c0_layers_n5_64x160', 64, 2, 4, 'BD', 5, 64, 160, {CHAIN: 0, RES: 0, WINO: 13, CONVT: 1}, env=C0),
    _c('w0_direct_64x160', 64, 2, 4, 'BD', 1, 64, 160, {WINO: 0, RES: 0, CHAIN: 0, R2: 13, ONESHOT: 2, Z: 2},
       env={'TG_CONV_WINO': '0'}),
]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def env_key(env):
    return tuple(sorted(env.items()))


def groups():
    """{env key: [cases]}, the default rule first."""
    out = {}
    for c in CASES:
        out.setdefault(env_key(c.env), []).append(c)
    return dict(sorted(out.items(), key=lambda kv: (len(kv[0]) > 0, kv[0])))


def configs():
    """{(nf, nb, scale, degradation): the smallest (h, w) the table runs it at} (fp32 cases)."""
    out = {}
    for c in CASES:
        if c.precision != 'fp32':
            continue
        k = (c.nf, c.nb, c.scale, c.degradation)
        if k not in out or c.h * c.w < out[k][0] * out[k][1]:
            out[k] = (c.h, c.w)
    return out
