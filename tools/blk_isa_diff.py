"""Device-assembly comparison of the blocked bf16 GEMM kernels of two builds (no GPU): regenerates the tables of profiles/blk_multitile_isa_diff.txt.

    cd w-hmr_amd/csrc    (of the parent tree and of this tree)
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result --cuda-device-only -S gemm_blk.hip -o gemm_blk.s      [+ -DWHMR_BLK_STAMPS]
    python tools/blk_isa_diff.py parent/gemm_blk.s new/gemm_blk.s

Per single-tile kernel: label .. .Lfunc_end with comments dropped, the symbol and the .LBB function numbers normalised, + the .amdhsa_kernel block;
"identical" = all of it equal.  Per multi-tile kernel: registers, scratch, and the s_waitcnt vmcnt between the first look-ahead LDS-DMA behind
the main loop and the last epilogue store (there must be none: a drain there puts the whole fetch in front of the stores)."""
import difflib
import re
import sys

def kernels(path):
    txt = open(path).read().split('\n')
    out = {}
    i = 0
    cur = None
    for ln in txt:
        m = re.match(r'^(_Z17gemm_blk16_kernelILi(\d)ELi(\d)ELi(\d)E(?:Lb([01])E)?EvT?\w*):\s*(;.*)?$', ln)
        if m and cur is None:
            cur = (int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5) or 0)); sym = m.group(1); body = []
            continue
        if cur is not None:
            if ln.startswith('.Lfunc_end'):
                out[cur] = {'sym': sym, 'body': body}; cur = None; continue
            s = ln.split(';')[0].rstrip()
            if not s.strip(): continue
            s = s.replace(sym, 'KSYM')
            s = re.sub(r'\.LBB\d+_', '.LBB_', s)
            body.append(s)
    # amdhsa blocks
    blocks = re.findall(r'\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel', '\n'.join(txt), re.S)
    for sym, blk in blocks:
        m = re.match(r'_Z17gemm_blk16_kernelILi(\d)ELi(\d)ELi(\d)E(?:Lb([01])E)?Ev', sym)
        if not m: continue
        k = (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4) or 0))
        lines = [l.split(';')[0].strip() for l in blk.split('\n') if l.strip()]
        out[k]['hsa'] = lines
        g = lambda f: int(re.search(r'\.amdhsa_%s (\d+)' % f, blk).group(1))
        out[k]['vgpr'], out[k]['sgpr'] = g('next_free_vgpr'), g('next_free_sgpr')
        out[k]['lds'], out[k]['scratch'] = g('group_segment_fixed_size'), g('private_segment_fixed_size')
        ma = re.search(r'\.amdhsa_accum_offset (\d+)', blk)
        out[k]['accum'] = int(ma.group(1)) if ma else -1
    return out
P, N = kernels(sys.argv[1]), kernels(sys.argv[2])
print('kernel<MI0,MI1,EPI>           instrs   vgpr   sgpr     lds  scratch  verdict')
nd = 0
for k in sorted(P):
    a, b = P[k], N[k]
    same = a['body'] == b['body'] and a['hsa'] == b['hsa']
    nd += not same
    ins = sum(1 for l in b['body'] if l.startswith('\t') and not l.strip().startswith('.'))
    v = 'identical' if same else 'DIFFERS (%d diff lines)' % sum(1 for l in difflib.unified_diff(a['body'], b['body'], lineterm='', n=0) if l[0] in '+-')
    print('gemm_blk16_kernel<%d,%d,%d>      %6d %6d %6d %7d %8d  %s' % (k[0], k[1], k[2], ins, b['vgpr'], b['sgpr'], b['lds'], b['scratch'], v))
print('%d kernels, %d differ' % (len(P), nd))
print()
print('multi-tile instantiations (new)   instrs   vgpr   sgpr     lds  scratch   single-tile: instrs vgpr sgpr')
for k in sorted(N):
    if k[3] == 1:
        b = N[k]; a = N[k[:3] + (0,)]
        ins = lambda x: sum(1 for l in x['body'] if l.startswith('\t') and not l.strip().startswith('.'))
        print('gemm_blk16_kernel<%d,%d,%d,MT>   %6d %6d %6d %7d %8d   %6d %4d %4d' % (k[0], k[1], k[2], ins(b), b['vgpr'], b['sgpr'], b['lds'], b['scratch'], ins(a), a['vgpr'], a['sgpr']))

print()
print('vmcnt waits between the first look-ahead DMA behind the main loop and the last epilogue store (multi-tile kernels of the new build)')
txt = open(sys.argv[2]).read()
for k in sorted(N):
    if k[3] != 1:
        continue
    sym = N[k]['sym']
    i = txt.index('\n' + sym + ':'); j = txt.index('.Lfunc_end', i)
    ins = [l.split(';')[0].strip() for l in txt[i:j].split('\n')[2:] if l.startswith('\t') and not l.strip().startswith('.') and not l.strip().startswith(';')]
    park = min(q for q, s in enumerate(ins) if s.startswith('global_load_lds_dword '))      # the parked values: only the look-ahead has dword DMAs
    lo = max(q for q in range(park) if ins[q].startswith(('s_barrier', 'v_mfma', 'ds_read_b64')))   # ... and its three stages follow the statistics reads
    st = [q for q, s in enumerate(ins) if q > park and 'global_store_dwordx4' in s]      # (the lab build's stamps are dwordx2 stores)
    dma = [q for q in range(lo, st[0]) if 'global_load_lds' in ins[q]]
    w = [ins[q] for q in range(dma[0], st[-1] + 1) if 's_waitcnt' in ins[q] and 'vmcnt' in ins[q]]
    print('gemm_blk16_kernel<%d,%d,%d,MT>   look-ahead DMAs %d, stores %d, vmcnt waits in between: %s' % (k[0], k[1], k[2], len(dma), len(st), len(w) if w else 'none'))
