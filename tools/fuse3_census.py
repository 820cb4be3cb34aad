#!/usr/bin/env python3
"""Static instruction census of the three-stage kernel (thetis_amd/csrc/swe2d_fuse.h: swe_fuse123_kernel), no GPU needed.

Cross-compiles csrc/swe2d_api_fuse.hip for gfx950 with the flags of thetis_amd/_build.py (device side only, to assembly), takes the text
of one instance and counts its instructions by class and by region.  The regions are cut at the kernel's barriers, in text order:

    prologue        entry .. barrier 1            tile record, connectivity, loads, the gather of the outside traces, LDS stores
    stage 1 body    barrier 1 .. barrier 2        cell integrals, three facets, finish (executed once per wave with a real cell)
    P1 store        barrier 2 .. barrier 3        stage 1's results into P1
    stage 2/3 body  barrier 3 .. end              the rolled loop: body, the barriers and LDS stores of s = 1, the stores of s = 2
                                                  (executed twice; the census counts its text once)

Counts are of the TEXT (wave-instructions per execution of a region if every branch falls through), not of a run.

    python tools/fuse3_census.py                       # this tree, instance <true,true,false>
    python tools/fuse3_census.py --src DIR             # another tree's thetis_amd/csrc (the parent commit, checked out elsewhere)
    python tools/fuse3_census.py --instance 1 1 1      # NONLIN LF SRC
    python tools/fuse3_census.py --functions           # + digest of every OTHER kernel's text in the unit (shared functions unchanged?)
"""
import argparse
import collections
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thetis_amd import _build  # noqa: E402

CLASSES = ['fp64', 'rsq/rcp/sqrt', 'cndmask/mov', 'int+addr VALU', 'VMEM', 'DS', 'waitcnt/barrier', 'SALU+branch']
REGIONS = ['prologue', 'stage 1 body', 'P1 store', 'stage 2/3 body']


def assembly(unit, csrc, defines=()):
    """device-side assembly of one translation unit, compiled as _build.py compiles it"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'unit.s')
        cmd = [_build.HIPCC] + _build.FLAGS + list(_build.UNIT_FLAGS.get(unit, [])) + ['-D' + d for d in defines] \
            + ['--cuda-device-only', '-S', os.path.join(csrc, unit), '-o', out]
        subprocess.check_call(cmd)
        return open(out).read(), ' '.join(cmd[:-3] + ['csrc/' + unit, '-o', 'unit.s'])


def functions(text):
    """name -> (instruction lines, trailer comment lines) of every function of an assembly file"""
    out, name, body = {}, None, []
    for line in text.splitlines():
        m = re.match(r'^([A-Za-z_][\w$.]*):', line)
        if m and not line.startswith('.L'):
            name, body = m.group(1), []
            out[name] = body
        elif name is not None:
            body.append(line)
    return out


def classify(mn):
    if mn.startswith(('s_waitcnt', 's_barrier')):
        return 'waitcnt/barrier'
    if mn.startswith(('buffer_', 'global_', 'flat_', 'scratch_')):
        return 'VMEM'
    if mn.startswith('ds_'):
        return 'DS'
    if mn.startswith('s_'):
        return 'SALU+branch'
    if mn.startswith(('v_rsq', 'v_rcp', 'v_sqrt')):
        return 'rsq/rcp/sqrt'
    if mn.startswith(('v_cndmask', 'v_mov', 'v_accvgpr', 'v_readlane', 'v_readfirstlane', 'v_writelane')):
        return 'cndmask/mov'
    if '_f64' in mn:
        return 'fp64'
    if mn.startswith('v_'):
        return 'int+addr VALU'
    return None


def census(body):
    """[region][class] counts, the mnemonic histogram of the non-FP64 VALU per region, resources"""
    counts = [collections.Counter() for _ in REGIONS]
    mnem = [collections.Counter() for _ in REGIONS]
    region, res, done = 0, {}, False
    for line in body:
        s = line.strip()
        for key, pat in (('vgprs', r'; NumVgprs: (\d+)'), ('agprs', r'; NumAgprs: (\d+)'), ('sgprs', r'; NumSgprs: (\d+)'),
                         ('scratch', r'; ScratchSize: (\d+)'), ('lds', r'; LDSByteSize: (\d+)'), ('code bytes', r'; codeLenInByte = (\d+)'),
                         ('occupancy', r'; Occupancy: (\d+)')):
            m = re.match(pat, s)
            if m:
                res[key] = int(m.group(1))
        if 'codeLenInByte' in s:
            done = True
        if done or not s or s.startswith((';', '.', '//')) or s.endswith(':'):
            continue
        mn = s.split()[0]
        c = classify(mn)
        if c is None:
            continue
        counts[region][c] += 1
        if c in ('cndmask/mov', 'int+addr VALU'):
            mnem[region][mn] += 1
        if mn == 's_barrier' and region < len(REGIONS) - 1:
            region += 1
    return counts, mnem, res


def table(counts, res):
    rows = ['{:<18}'.format('class') + ''.join('{:>16}'.format(r) for r in REGIONS)]
    for c in CLASSES:
        rows.append('{:<18}'.format(c) + ''.join('{:>16}'.format(counts[i][c]) for i in range(len(REGIONS))))
    valu = [sum(counts[i][c] for c in CLASSES[:4]) for i in range(len(REGIONS))]
    rows.append('{:<18}'.format('VALU total') + ''.join('{:>16}'.format(x) for x in valu))
    rows.append('resources: ' + ', '.join('{} {}'.format(k, v) for k, v in res.items()))
    return '\n'.join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--src', default=_build.CSRC, help="the csrc directory to compile (default: this tree's)")
    ap.add_argument('--instance', nargs=3, type=int, default=[1, 1, 0], metavar=('NONLIN', 'LF', 'SRC'))
    ap.add_argument('--mnemonics', action='store_true', help='the non-FP64 VALU mnemonics per region')
    ap.add_argument('--functions', nargs='*', metavar='UNIT', default=None,
                    help='sha256 of the instruction text of every other kernel of these units (default: the three that see swe2d_flow.h)')
    args = ap.parse_args()
    text, cmd = assembly('swe2d_api_fuse.hip', args.src)
    fns = functions(text)
    want = 'swe_fuse123_kernelILb{}ELb{}ELb{}EE'.format(*args.instance)
    name = [n for n in fns if want in n and not n.endswith('.kd')]
    assert len(name) == 1, name
    counts, mnem, res = census(fns[name[0]])
    print('# ' + cmd)
    print('# ' + name[0])
    print(table(counts, res))
    if args.mnemonics:
        for i, r in enumerate(REGIONS):
            print('{}: '.format(r) + ', '.join('{} {}'.format(m, n) for m, n in mnem[i].most_common()))
    if args.functions is not None:
        for unit in args.functions or ['swe2d_api_fuse.hip', 'swe2d_k_flow.hip', 'swe2d_k_flow_wd.hip']:
            ufns = fns if unit == 'swe2d_api_fuse.hip' else functions(assembly(unit, args.src)[0])
            print('# ' + unit)
            for n in sorted(ufns):
                if 'swe_fuse123_kernel' in n or n.endswith('.kd') or 'kernel' not in n:
                    continue
                ins = [re.sub(r'\.LBB\d+_', '.LBB_', ln.split(';')[0].strip()) for ln in ufns[n]]
                ins = [ln for ln in ins if ln and not ln.startswith('.') and not ln.endswith(':')]
                print('{}  {:6d} instructions  {}'.format(hashlib.sha256('\n'.join(ins).encode()).hexdigest()[:16], len(ins), n))


if __name__ == '__main__':
    main()
