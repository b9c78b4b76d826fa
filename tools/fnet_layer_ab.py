"""Lab: FNet layers with a pool / x2 up-sampling neighbour at the batched flow pass's shapes (n frame pairs of 134x320), three ways:
direct kernel + glue launch, Winograd form + glue launch, Winograd form with the glue folded in (POOL / UP2).  cout = 32
runs the 32-channel workgroup.  Usage: python tools/fnet_layer_ab.py [pairs]   (EXPERIMENTS.md: flow pass entry)"""
import os, sys, torch, numpy as np
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
    return min(ts), float(np.median(ts))
n = int(sys.argv[1]) if len(sys.argv) > 1 else 8
A = ops.ACT_LRELU02
def case(name, cin, cout, h, w, pool, up2):
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
    d = (direct() - wino_fused()).abs().max().item()
    print(f'{name} n={n} {cin}->{cout} {h}x{w}: direct+glue {timeit(direct)}  wino+glue {timeit(wino_sep)}  wino fused {timeit(wino_fused)} us (min, median)  maxdiff {d:.2e}', flush=True)
case('encoder1.2+pool', 32, 32, 134, 320, True, False)
case('flow.0<-up2', 64, 32, 128, 320, False, True)
case('decoder2.0<-up2', 256, 128, 32, 80, False, True)
case('decoder3.0<-up2', 128, 64, 64, 160, False, True)
case('encoder2.2+pool(66)', 64, 64, 66, 160, True, False)
