#!/usr/bin/env python3
"""Compare the device code of two trees kernel by kernel, as the product build compiles it:

  python tools/isa/compare_code_objects.py dump OUTDIR [--root TREE] [--units stem,stem,...] [--flags '-DX ...'] [--jobs N]
  python tools/isa/compare_code_objects.py compare PARENT_DIR BRANCH_DIR [--json OUT.json]

`dump` compiles every unit of serl_amd.build (all_units(): UNITS and UNITS_BESIDE) of TREE (default: this tree) device-only for gfx950 with the product's flags down to the assembly the
compiler hands its assembler (-S, no line tables) and writes OUTDIR/<unit>.json: per function symbol the text of its body with comments stripped (kept
whole in OUTDIR/<unit>.s for diff), its SHA-256, and for kernels the resource numbers of the code-object metadata (VGPR, AGPR, SGPR, spills, private
segment, LDS).  The assembly, not a disassembly of the linked code object: there a call of a function of the unit is a pc-relative displacement that moves
with the size of every function in between, so that each caller differs as soon as one function does; here it is the callee's name.  `compare` lists
every symbol as identical (same text, same resources) or different, with both sets of resource numbers.  The texts are compared whole: the tool knows
no instruction."""
import argparse, hashlib, importlib.util, json, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KEYS = ('vgpr_count', 'agpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size', 'group_segment_fixed_size')


def load_build(root):
    spec = importlib.util.spec_from_file_location('serl_build_' + hashlib.md5(root.encode()).hexdigest(), os.path.join(root, 'serl_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dump_unit(B, unit, outdir, flags=()):
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, 'u.s')
        r = subprocess.run(B.compile_argv(unit, asm, list(flags) + ['--cuda-device-only', '-S']), capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError('hipcc failed for %s:\n%s' % (unit, r.stderr[-3000:]))
        text = open(asm).read()
    res = {}
    meta = text[text.index('.amdgpu_metadata'):]
    for blk in re.findall(r'- \.agpr_count.*?(?=\n\s+- \.agpr_count|\Z)', meta, re.S):
        nm = re.search(r'^    \.name:\s+(\S+)', blk, re.M)      # (the kernel's own keys, the block's first behind its '- ': the arguments' names sit deeper)
        res[nm.group(1)] = {k: int(m.group(1)) for k in KEYS for m in [re.search(r'^(?:    |- )\.%s:\s+(\d+)' % k, blk, re.M)] if m}
    funcs, cur = {}, None
    for ln in text.split('\n'):
        m = re.match(r'^([A-Za-z_$][\w$.]*):\s+; @', ln)
        if m:
            cur = funcs.setdefault(m.group(1), [])
        elif re.match(r'^\.Lfunc_end\d+:', ln):
            cur = None
        elif cur is not None:
            ln = re.sub(r'\s*;.*$', '', ln).strip()      # (comments: block names, the register pressure of a region)
            if ln:
                cur.append(ln)
    out = {}
    with open(os.path.join(outdir, unit + '.s'), 'w') as f:
        for name, body in funcs.items():
            body = '\n'.join(body)
            f.write('<%s>:\n%s\n\n' % (name, body))
            out[name] = dict(kernel=name in res, lines=body.count('\n') + 1, sha256=hashlib.sha256(body.encode()).hexdigest(), resources=res.get(name))
    missing = [k for k in res if k not in out]
    if missing or not res:
        raise RuntimeError('%s: kernels in the metadata without text: %s' % (unit, missing))
    with open(os.path.join(outdir, unit + '.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    return unit


def cmd_dump(a):
    B = load_build(os.path.abspath(a.root))
    units = a.units.split(',') if a.units else list(B.all_units() if hasattr(B, 'all_units') else B.UNITS)      # (a tree from before all_units: its UNITS)
    os.makedirs(a.outdir, exist_ok=True)
    with ThreadPoolExecutor(max_workers=a.jobs) as ex:
        for u in ex.map(lambda u: dump_unit(B, u, a.outdir, a.flags.split()), units):
            print(u, flush=True)


def cmd_compare(a):
    table, ndiff = {}, 0
    units = sorted(f[:-5] for f in os.listdir(a.parent) if f.endswith('.json'))
    if units != sorted(f[:-5] for f in os.listdir(a.branch) if f.endswith('.json')):
        sys.exit('the two dumps hold different units')
    for u in units:
        p, b = (json.load(open(os.path.join(d, u + '.json'))) for d in (a.parent, a.branch))
        row = {}
        for name in sorted(set(p) | set(b)):
            x, y = p.get(name), b.get(name)
            if x and y and x['sha256'] == y['sha256'] and x['resources'] == y['resources']:
                row[name] = 'identical'
            else:
                ndiff += 1
                row[name] = dict(parent=x and dict(lines=x['lines'], resources=x['resources']),
                                 branch=y and dict(lines=y['lines'], resources=y['resources']))
        table[u] = row
        d = [n for n, v in row.items() if v != 'identical']
        print('%-28s %3d symbols  %s' % (u, len(row), 'identical' if not d else 'DIFFERENT: ' + ', '.join(d)))
    print('%d units, %d symbols differ' % (len(units), ndiff))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(table, f, indent=1, sort_keys=True)
    return ndiff


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest='cmd', required=True)
    d = sub.add_parser('dump')
    d.add_argument('outdir'); d.add_argument('--root', default=HERE_ROOT); d.add_argument('--units', default=''); d.add_argument('--flags', default='', help='extra hipcc flags, space separated'); d.add_argument('--jobs', type=int, default=min(16, os.cpu_count() or 8))
    c = sub.add_parser('compare')
    c.add_argument('parent'); c.add_argument('branch'); c.add_argument('--json', default='')
    a = ap.parse_args()
    cmd_dump(a) if a.cmd == 'dump' else cmd_compare(a)
