#!/usr/bin/env python3
"""Static instruction counts of the kernels of a translation unit (hipcc -S): total, vector, scalar, LDS, vector memory, branches.
usage: python tools/isa_count.py [bf_kernels_sp.hip] [name filter] [--dump DIR]
--dump DIR also writes each listed kernel's normalised body (no comments, no directives, local labels renumbered in order of appearance) to a
file of its own under DIR, so that two trees are compared with diff -r."""
import os, re, subprocess, sys, collections
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
dump = None
if "--dump" in args:
    i = args.index("--dump")
    dump = args[i + 1]
    del args[i:i + 2]
    os.makedirs(dump, exist_ok=True)
src = args[0] if len(args) > 0 else "bf_kernels_sp.hip"
flt = args[1] if len(args) > 1 else ""
out = "/tmp/isa_%s.s" % os.path.basename(src)
subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                       os.path.join(ROOT, "blingfire_amd", "csrc", src), "-o", out] + (["-DBF_EXPERIMENTS"] if os.environ.get("BF_EXPERIMENTS") else []), stderr=subprocess.DEVNULL)
s = open(out).read()
for m in re.finditer(r'^(_ZN3bfa\S+):\s*;', s, re.M):
    full = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
    name = re.sub(r"\(.*", "", full).replace("bfa::", "")
    if flt not in name: continue
    end = s.index('.Lfunc_end', m.end())
    c = collections.Counter()
    body, labels = [], {}
    for l in s[m.end():end].split('\n'):
        l = l.split(';')[0].strip()
        if l.endswith(':') or not l.startswith('.'):
            body.append(re.sub(r'\.L\w+', lambda t: labels.setdefault(t.group(0), ".L%d" % len(labels)), l))
        if not l or l.startswith('.') or l.endswith(':'): continue
        op = l.split()[0]
        c['total'] += 1
        if op.startswith('v_readlane') or op.startswith('v_writelane') or op.startswith('v_readfirstlane'): c['lane'] += 1
        if op.startswith('v_'): c['valu'] += 1
        elif op.startswith('s_cbranch') or op.startswith('s_branch'): c['branch'] += 1
        elif op.startswith('s_'): c['salu'] += 1
        elif op.startswith('ds_'): c['lds'] += 1
        elif op.startswith(('global_', 'flat_', 'buffer_', 'scratch_')): c['vmem'] += 1; c['scratch'] += op.startswith('scratch_')
    if dump:
        open(os.path.join(dump, re.sub(r'\W+', '_', name).strip('_') + ".s"), "w").write("\n".join(b for b in body if b) + "\n")
    print("%-60s total %5d valu %5d salu %5d branch %4d lds %4d vmem %4d lane-moves %4d scratch %3d" % (name[:60], c['total'], c['valu'], c['salu'], c['branch'], c['lds'], c['vmem'], c['lane'], c['scratch']))
