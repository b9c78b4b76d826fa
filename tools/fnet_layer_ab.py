"""Lab: FNet layers with a pool / x2 up-sampling neighbour at the batched flow pass's shapes (n frame pairs of 134x320):
direct kernel + glue launch, Winograd form + glue launch, Winograd form with the glue folded in (POOL / UP2), and -- for the
three readers of an up-sampling -- the factored form (tg_upconv.hip: tap GEMM at the low resolution + combine), whole
and per launch.  cout = 32 runs the 32-channel workgroup.  40 launches back to back per timing.
Usage: python tools/fnet_layer_ab.py [pairs ...] [--json PATH]   (EXPERIMENTS.md: flow pass entries)"""
import json, os, sys, torch, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tecogan_pytorch_amd import ops, _lib
def rnd(*s): return (torch.rand(*s, device='cuda') * 2 - 1)
def timeit(f, it=40):
    for _ in range(5): f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(it): f()
        b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / it)
    return round(min(ts), 1), round(float(np.median(ts)), 1)
args = sys.argv[1:]
jpath = args[args.index('--json') + 1] if '--json' in args else None
pairs = [int(a) for a in args if a.isdigit()] or [8]
A = ops.ACT_LRELU02
rows = []
def case(name, n, cin, cout, h, w, pool, up2):
    wt = rnd(cout, cin, 3, 3) / (3 * cin ** 0.5); b = rnd(cout)
    pk, _, _, ocb = ops.pack_conv3x3(wt); u = ops.pack_conv3x3_wino(wt)
    src = rnd(n, cin, h // 2, w // 2) if up2 else rnd(n, cin, h, w)
    def direct():
        x = ops.upsample(src, 2, ops.UP_BILINEAR) if up2 else src
        y = ops.conv3x3(x, pk, b, cin, cout, ocb, A, ksplit=1)
        return ops.maxpool2(y) if pool else y
    def wino_sep():
        x = ops.upsample(src, 2, ops.UP_BILINEAR) if up2 else src
        y = ops.conv3x3_wino(x, u, b, cin, cout, A)
        return ops.maxpool2(y) if pool else y
    def wino_fused():
        return ops.conv3x3_wino(src, u, b, cin, cout, A, pool=pool, up2=up2)
    row = dict(layer=name, pairs=n, cin=cin, cout=cout, h=h, w=w, direct_glue=timeit(direct), wino_glue=timeit(wino_sep),
               wino_fused=timeit(wino_fused), maxdiff_wino_fused=(direct() - wino_fused()).abs().max().item())
    if up2:
        ap = ops.pack_upconv(wt)
        z = torch.empty(n, 9 * cout, h // 2, w // 2, device='cuda'); y = torch.empty(n, cout, h, w, device='cuda')
        row.update(upsample=timeit(lambda: ops.upsample(src, 2, ops.UP_BILINEAR)),
                   factored=timeit(lambda: (ops.upconv_tap_gemm(src, ap, cin, cout, z=z), ops.upconv_combine(z, b, cout, A, out=y))),
                   tap_gemm=timeit(lambda: ops.upconv_tap_gemm(src, ap, cin, cout, z=z)),
                   combine=timeit(lambda: ops.upconv_combine(z, b, cout, A, out=y)),
                   maxdiff_factored=(direct() - ops.upconv3x3(src, ap, b, cin, cout, A)).abs().max().item(),
                   prefers_wino=_lib.lib().tg_conv3x3_prefers_wino(n, cin, cout, h, w),
                   prefers_upconv=_lib.lib().tg_upconv_prefers(n, cin, cout, h // 2, w // 2))
        for k in (1, 2, 4):      # the same two launches per group of k pairs: z of a group stays in the caches
            if k < n and n % k == 0:
                def grouped():
                    for i in range(0, n, k):
                        ops.upconv_tap_gemm(src[i:i + k], ap, cin, cout, z=z[:k])
                        ops.upconv_combine(z[:k], b, cout, A, out=y[i:i + k])
                row['factored_groups_of_%d' % k] = timeit(grouped)
    rows.append(row)
    print(' '.join('%s %s' % kv for kv in row.items()) + '   (us: min, median)', flush=True)
for n in pairs:
    if n == 8:
        case('encoder1.2+pool', n, 32, 32, 134, 320, True, False)
        case('encoder2.2+pool(66)', n, 64, 64, 66, 160, True, False)
    case('flow.0<-up2', n, 64, 32, 128, 320, False, True)
    case('decoder2.0<-up2', n, 256, 128, 32, 80, False, True)
    case('decoder3.0<-up2', n, 128, 64, 64, 160, False, True)
if jpath:
    json.dump(rows, open(jpath, 'w'), indent=1)
