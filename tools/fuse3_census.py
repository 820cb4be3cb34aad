#!/usr/bin/env python3
"""Static instruction census of the three-stage kernel (thetis_amd/csrc/swe2d_fuse.h: swe_fuse123_kernel), no GPU needed.

Cross-compiles csrc/swe2d_api_fuse.hip for gfx950 with the flags of thetis_amd/_build.py (device side only, to assembly), takes the text
of one instance and counts its instructions by class and by region.  The regions are cut at the kernel's barriers, in text order:

    prologue        entry .. barrier 1            tile record, connectivity, loads, the gather of the outside traces, LDS stores
    stage 1 body    barrier 1 .. barrier 2        cell integrals, three facets, finish (executed once per wave with a real cell)
    P1 store        barrier 2 .. barrier 3        stage 1's results into P1
    stage 2/3 body  barrier 3 .. end              the rolled loop: body, the barriers and LDS stores of s = 1, the stores of s = 2
                                                  (executed twice; the census counts its text once)

Since round 22 stages 2 and 3 are two copies of one body (the loop is peeled); the text then has six regions,
    ... stage 2 body (barrier 3 .. 4), P1 store 2 (barrier 4 .. 5), stage 3 body (barrier 5 .. end: body and the stores of U(3)),
told from the rolled text by the FP64 instructions behind the fifth barrier (the rolled loop has only the stores of s = 2 there).

Counts are of the TEXT (wave-instructions per execution of a region if every branch falls through), not of a run.

    python tools/fuse3_census.py                       # this tree, instance <true,true,false>
    python tools/fuse3_census.py --src DIR             # another tree's thetis_amd/csrc (the parent commit, checked out elsewhere)
    python tools/fuse3_census.py --instance 1 1 1      # NONLIN LF SRC
    python tools/fuse3_census.py --functions           # + digest of every OTHER kernel's text in the unit (shared functions unchanged?)
    python tools/fuse3_census.py --paths               # + each stage body split into the path a wave without a wall cell takes and the rest

--paths cuts a stage body at its branches.  The outermost forward branch of a body is the activity test (real / act).  The largest
forward branch inside it is `bmarkers != 0` of swe_tri_finish: what it skips is the BOUNDARY PASS.  Short blocks behind a forward
SCALAR branch (s_cbranch_scc* / _vcc*) outside the boundary pass are the wave-uniform blocks (the zeroing of a boundary facet's flux where the
kernel asks for it, swe_tri_facet<.., WAVEB>): skipped by a wave no lane of which has a boundary facet.  The rest is the STRAIGHT-LINE
PATH, the text a wave of a tile without wall cells executes.  Every non-FP64 VALU instruction of that path is listed with the source
construct it belongs to, told from its mnemonic and operands:
    zeroing           v_mov_b64 v[..], 0                                  the six fluxes of a boundary facet (swe_tri_facet)
    facet tests       v_and_b32 0xff00 / 0xff0000, v_cmp_{eq,ne}_u32 .. 0, BYTE_0 compares, v_mov_b32 v, 0 for those: bnd per facet, bmarkers != 0
    trace addresses   v_and_b32 0xffff, v_lshrrev_b32 16                   the two 16-bit LDS addresses of a facet's tr word
    store addresses   64-bit integer arithmetic (v_lshl_add_u64, v_mad_u64_u32, v_lshlrev_b64, v_add_co / v_addc_co, v_ashrrev_i32 .. 31)
    loop copies       v_mov_b64 / v_mov_b32 register to register          u = ou of the s == 1 arm, values carried round the rolled loop
    activity tests    signed compares with the role, v_subrev_u32, v_readlane
    other             whatever is left
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
ROLLED = ['prologue', 'stage 1 body', 'P1 store', 'stage 2/3 body']
PEELED = ['prologue', 'stage 1 body', 'P1 store', 'stage 2 body', 'P1 store 2', 'stage 3 body']
REGIONS = list(ROLLED)
BODIES = [1, 3]                                              # the regions that hold a stage body


def detect_regions(body):
    """sets REGIONS / BODIES for the text of one instance: peeled when a stage body follows the fifth barrier"""
    barriers, fp64_behind = 0, 0
    for line in body:
        s = line.strip()
        if 'codeLenInByte' in s:
            break
        if not s or s.startswith((';', '.', '//')) or s.endswith(':'):
            continue
        mn = s.split()[0]
        barriers += mn == 's_barrier'
        fp64_behind += barriers >= 5 and '_f64' in mn
    REGIONS[:] = PEELED if fp64_behind >= 200 else ROLLED
    BODIES[:] = [1, 3, 5] if fp64_behind >= 200 else [1, 3]


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


CONSTRUCTS = ['zeroing', 'facet tests', 'trace addresses', 'store addresses', 'loop copies', 'activity tests', 'other']


def construct(mn, ops):
    """the source construct of a non-FP64 VALU instruction of the straight-line path (see the module's text)"""
    first = ops.split(',')[0].strip() if ops else ''
    rest = [o.strip() for o in ops.split(',')[1:]]
    if mn.startswith('v_mov_b64'):
        return 'zeroing' if rest and rest[0] == '0' else 'loop copies'
    if mn.startswith('v_mov_b32'):
        if rest and rest[0].startswith('v'):
            return 'loop copies'
        return 'facet tests' if rest and rest[0] == '0' else 'other'
    if mn.startswith('v_and_b32') and rest and rest[0] in ('0xff00', '0xff0000', '0xff'):
        return 'facet tests'
    if (mn.startswith('v_and_b32') and rest and rest[0] == '0xffff') or (mn.startswith('v_lshrrev_b32') and rest and rest[0] == '16'):
        return 'trace addresses'
    if mn.startswith(('v_lshl_add_u64', 'v_mad_u64_u32', 'v_lshlrev_b64', 'v_add_co_u32', 'v_addc_co_u32')) or \
            (mn.startswith('v_ashrrev_i32') and rest and rest[0] == '31'):
        return 'store addresses'
    if mn.startswith(('v_cmp_lt_i32', 'v_cmp_gt_i32', 'v_cmp_le_i32', 'v_cmp_ge_i32', 'v_subrev_u32', 'v_sub_u32', 'v_readlane')):
        return 'activity tests'
    if mn.startswith(('v_cmp_eq_u32', 'v_cmp_ne_u32')):
        return 'facet tests'
    return 'other'


def split_paths(body):
    """per region with a stage body: the VALU counts of the straight-line path, of the wave-uniform blocks and of the boundary pass,
    and the listing [(mnemonic, operands, construct)] of the straight-line path's non-FP64 VALU"""
    # the instruction lines and labels of the function, by region
    items, region = [], 0                                    # (region, kind, text): kind 'label' | 'ins'
    for line in body:
        s = line.split(';')[0].strip()
        if 'codeLenInByte' in line:
            break
        if not s or s.startswith(('.', '//')) and not s.endswith(':'):
            continue
        if s.endswith(':'):
            items.append((region, 'label', s[:-1]))
            continue
        items.append((region, 'ins', s))
        if s.split()[0] == 's_barrier' and region < len(REGIONS) - 1:
            region += 1
    where = {t: i for i, (_, k, t) in enumerate(items) if k == 'label'}
    out = {}
    for r in BODIES:
        idx = [i for i, it in enumerate(items) if it[0] == r]
        lo, hi = idx[0], idx[-1]
        fwd = []                                             # (start, end, mnemonic) of every forward conditional branch of the region
        for i in idx:
            if items[i][1] == 'ins' and items[i][2].startswith('s_cbranch'):
                mn, target = items[i][2].split()[:2]
                j = where.get(target)
                if j is not None and j > i:
                    fwd.append((i, min(j, hi + 1), mn))
        execz = [b for b in fwd if b[2] == 's_cbranch_execz']
        act = max(execz, key=lambda b: b[1] - b[0])
        inner = [b for b in execz if b[0] > act[0] and b[1] <= act[1]]
        bpass = max(inner, key=lambda b: b[1] - b[0])
        uniform = [b for b in fwd if b[2].startswith(('s_cbranch_scc', 's_cbranch_vcc')) and act[0] < b[0] < act[1] and b[1] - b[0] < 40 and not (bpass[0] < b[0] < bpass[1])]
        counts = {'straight': collections.Counter(), 'uniform': collections.Counter(), 'boundary': collections.Counter()}
        listing = []
        for i in idx:
            if items[i][1] != 'ins':
                continue
            mn, _, ops = items[i][2].partition(' ')
            c = classify(mn)
            if c not in CLASSES[:4]:
                continue
            part = 'boundary' if bpass[0] < i < bpass[1] else ('uniform' if any(b[0] < i < b[1] for b in uniform) else 'straight')
            counts[part][c] += 1
            if part == 'straight' and c in ('cndmask/mov', 'int+addr VALU'):
                listing.append((mn, ops.strip(), 'other' if mn.startswith('v_cndmask') else construct(mn, ops.strip())))
        out[r] = (counts, listing, len(uniform))
    return out


def paths_report(body):
    rows = []
    for r, (counts, listing, n_uniform) in split_paths(body).items():
        tot = {k: sum(v.values()) for k, v in counts.items()}
        rows.append('{}: straight-line path {} VALU ({} FP64), wave-uniform blocks {} VALU in {} blocks, boundary pass {} VALU ({} FP64)'.format(
            REGIONS[r], tot['straight'], counts['straight']['fp64'], tot['uniform'], n_uniform, tot['boundary'], counts['boundary']['fp64']))
        by = collections.Counter(c for _, _, c in listing)
        rows.append('  non-FP64 VALU of the straight-line path: ' + ', '.join('{} {}'.format(c, by[c]) for c in CONSTRUCTS))
        for c in CONSTRUCTS:
            for mn, ops, cc in listing:
                if cc == c:
                    rows.append('    {:<16} {} {}'.format(c, mn, ops))
    return '\n'.join(rows)


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
    ap.add_argument('--paths', action='store_true', help='each stage body split into straight-line path, wave-uniform blocks and boundary pass')
    ap.add_argument('--functions', nargs='*', metavar='UNIT', default=None,
                    help='sha256 of the instruction text of every other kernel of these units (default: the three that see swe2d_flow.h)')
    args = ap.parse_args()
    text, cmd = assembly('swe2d_api_fuse.hip', args.src)
    fns = functions(text)
    want = 'swe_fuse123_kernelILb{}ELb{}ELb{}EE'.format(*args.instance)
    name = [n for n in fns if want in n and not n.endswith('.kd')]
    assert len(name) == 1, name
    detect_regions(fns[name[0]])
    counts, mnem, res = census(fns[name[0]])
    print('# ' + cmd)
    print('# ' + name[0])
    print(table(counts, res))
    if args.mnemonics:
        for i, r in enumerate(REGIONS):
            print('{}: '.format(r) + ', '.join('{} {}'.format(m, n) for m, n in mnem[i].most_common()))
    if args.paths:
        print(paths_report(fns[name[0]]))
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
