"""Static instruction census of the resident launch's hand-over (tg_conv3x3_wino_res.hip), no GPU needed.
  hipcc <build.sh's FLAGS> -fno-slp-vectorize --cuda-device-only -S tg_conv3x3_wino_res.hip -o res.s
  python tools/wres_census.py res.s
Counts VALU / SALU / branch / memory instructions of conv3x3_wino_resident_kernel between the layer loop's workgroup
barrier (the third s_barrier of the kernel) and the boundary waves' arrival (ds_add_u32), split at the first ring load:
`geometry` is what a boundary wave executes before it can request its first ring pixel, `fetch` the loads, tag checks,
LDS stores and the poll bookkeeping behind it.  Static counts of the text, not executed instructions."""
import collections
import json
import re
import sys


def kind(op):
    if op.startswith('s_cbranch') or op == 's_branch':
        return 'branch'
    if op.startswith(('s_waitcnt', 's_nop', 's_sleep', 's_barrier')):
        return 'wait'
    if op.startswith('s_'):
        return 'salu'
    if op.startswith(('buffer_', 'global_', 'ds_', 'flat_')):
        return 'mem'
    if op.startswith('v_'):
        return 'valu'
    return 'other'


def main(path):
    ops, inside = [], False
    for ln in open(path):
        if re.match(r'_\w*conv3x3_wino_resident_kernel\w*:', ln):
            inside = True
        if not inside:
            continue
        m = re.match(r'\s+([a-z][a-z0-9_]+)', ln)
        if m:
            ops.append(m.group(1))
            if m.group(1) == 's_endpgm':
                break
    barriers = [i for i, o in enumerate(ops) if o == 's_barrier']
    start = barriers[2]
    end = next(i for i in range(start, len(ops)) if ops[i] == 'ds_add_u32')
    first = next(i for i in range(start, end) if ops[i] == 'buffer_load_dwordx4')
    out = {}
    for name, (a, b) in {'geometry': (start + 1, first), 'fetch': (first, end)}.items():
        c = collections.Counter(kind(o) for o in ops[a:b])
        out[name] = {k: c.get(k, 0) for k in ('valu', 'salu', 'branch', 'mem', 'wait')}
    print(json.dumps(out))


if __name__ == '__main__':
    main(sys.argv[1])
