"""Compile the HIP extension for gfx950, in-tree (serl_amd/csrc/libserl_amd.so).

hipcc cross-compiles without a GPU, so this runs in the CPU-only build container; the built .so is
git-ignored but travels to the GPU box with the repo snapshot.
"""
import os, subprocess, sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(CSRC, 'libserl_amd.so')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
# index = serl_dyn_code (include/serl_amd.h): csrc/serl_variant.h turns -DSERL_DYN=<code> into the variant's names and generated files
VARIANTS = ['nominal', 'ice', 'cg_timed', 'gust', 'test']
# kernel families: csrc/family_<f>.hip, compiled once per code variant into build/rollout_<f>_<variant>.o (the lane family: rollout_<variant>.o)
FAMILIES = ['lane', 'lanenz', 'lanern', 'laneg', 'lanegn', 'lanegt', 'lanegtn', 'venvw', 'venvwr', 'wave', 'wavern', 'half', 'team', 'teamr', 'teams2', 'team2', 'team2s', 'team4']      # (lanenz: the env kernels of the lane units with the in-kernel noise generator; venvw: the env kernels with one wavefront per env; venvwr: their rollout kernels; lanern / wavern: the population rollout kernels of the lane / wave units with the generator; laneg / lanegn: the lane population kernel around the general lane actor -- kernel_hint LANEG --, plain / with the generator; lanegt / lanegtn: the same two over the regrouped copy of the weights -- serl_rollout_regrouped)
# object stem -> (source, defines)
UNITS = {s: (s + '.hip', []) for s in ('serl_capi', 'serl_ga', 'serl_metrics', 'serl_distill', 'serl_td3', 'serl_noise')}
UNITS.update({('rollout_' if f == 'lane' else 'rollout_%s_' % f) + v: ('family_%s.hip' % f, ['-DSERL_DYN=%d' % code])
              for f in FAMILIES for code, v in enumerate(VARIANTS)})
UNITS['rollout_team4_mixed'] = ('rollout_team4_mixed.hip', [])      # (two code variants in one code object)
# units added beside the table above, which tests pin entry by entry (the way _capi._Table keeps its later entries): compiled and linked like the others
UNITS_BESIDE = {'serl_ga_sens': ('serl_ga_sens.hip', []),            # serl_ga_sensitivity_general, built from the learner's phases (serl_td3_core.inc)
                'serl_ga_nov': ('serl_ga_nov.hip', [])}              # serl_ga_novelty_general, likewise


def all_units():
    """object stem -> (source, defines) of every unit of the library: UNITS and UNITS_BESIDE"""
    return dict(UNITS, **UNITS_BESIDE)
# -ffp-contract=off: the IEEE-754 operation order of the reference binary is part of the contract (no FMA fusion).
# -disable-machine-licm: the model evaluation is inlined into the ODE5 stage loop; hoisting its ~110 f64 literals
# out of the loop (2 SGPRs each) makes them spill -- rematerialising them at use is cheaper.
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-fPIC', '-Wno-unused-value',
         '-DCITW_EVAL_INLINE=__forceinline__', '-mllvm', '-disable-machine-licm']


def _deps():
    out = []
    for root, _, files in os.walk(CSRC):
        for f in files:
            if f.endswith(('.hip', '.h', '.inc')):
                out.append(os.path.join(root, f))
    out.append(os.path.join(os.path.dirname(HERE), 'include', 'serl_amd.h'))
    return out


def source_hash():
    """SHA-256 over the kernel sources (serl_amd/csrc/**.hip|.h|.inc, include/serl_amd.h, the build flags): what a measurement of the library belongs to.
    tools/profile_round.sh records it next to the counters it collects, tools/distill_profiles.py stores it in profiles/pmc_current.json and
    floors_current.json, and bench.py quotes those numbers only while it still matches the tree it runs from."""
    import hashlib
    h = hashlib.sha256(' '.join(FLAGS).encode())
    for f in sorted(_deps()):
        if os.sep + 'build' + os.sep in f or '_role_isa' in f or '_exp' in os.path.basename(f):
            continue
        h.update(os.path.relpath(f, os.path.dirname(HERE)).encode())
        h.update(open(f, 'rb').read())
    return h.hexdigest()


def unit_stem(unit):
    """The object stem of a unit named by its stem or, as before the family sources, by '<stem>.hip' (e.g. 'rollout_team4_nominal.hip': build/rollout_team4_nominal.o, family_team4.hip with -DSERL_DYN=0)."""
    stem = unit[:-4] if unit.endswith('.hip') else unit
    if stem not in all_units():
        raise KeyError('unknown unit %r (one of: %s)' % (unit, ', '.join(all_units())))
    return stem


def compile_argv(unit, out, extra_flags=(), flags=None):
    """The hipcc command line that compiles `unit` (unit_stem) into `out`: the product's FLAGS (or `flags`), the unit's defines, `extra_flags`."""
    src, defines = all_units()[unit_stem(unit)]
    return [HIPCC] + list(FLAGS if flags is None else flags) + defines + list(extra_flags) + ['-c', os.path.join(CSRC, src), '-o', out]


def obj_path(unit, tag=''):
    return os.path.join(CSRC, 'build', unit_stem(unit) + tag + '.o')


def _compile(units, tag, extra_flags, verbose=False):
    os.makedirs(os.path.join(CSRC, 'build'), exist_ok=True)

    def cc(unit):
        obj = obj_path(unit, tag)
        r = subprocess.run(compile_argv(unit, obj, extra_flags), capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError('hipcc failed for %s:\n%s' % (unit, r.stderr[-4000:]))
        if verbose and r.stderr:
            print(r.stderr, file=sys.stderr)
        return obj
    with ThreadPoolExecutor(max_workers=min(len(units), max(4, 4 * (os.cpu_count() or 8)))) as ex:      # (hipcc spends most of its time waiting on its own sub-processes)
        return list(ex.map(cc, units))


def link(path, objs):
    r = subprocess.run([HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', path] + list(objs), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError('link failed:\n' + r.stderr[-4000:])
    return path


def _fresh(path, deps):
    return os.path.exists(path) and all(os.path.getmtime(path) >= os.path.getmtime(d) for d in deps)


def build(force=False, verbose=False, extra_flags=(), lib=None, tag=''):
    """extra_flags / lib / tag build a variant next to the product library (e.g. the phase-profiling build:
    extra_flags=['-DCITW_PROFILE'], lib='libserl_amd_prof.so', tag='_prof')."""
    path = os.path.join(CSRC, lib) if lib else LIB
    if not force and _fresh(path, _deps()):
        return path
    return link(path, _compile(list(all_units()), tag, extra_flags, verbose))


JITTER_LIB = 'libserl_amd_jitter.so'
TEAM_UNITS = [u for u in UNITS if u.startswith('rollout_team')]


def build_variant(lib, tag, extra_flags, units, force=False):
    """A library next to the product: `units` recompiled with `extra_flags` (objects build/<unit><tag>.o), every other object the
    product's own."""
    build()
    path = os.path.join(CSRC, lib)
    if not force and _fresh(path, _deps() + [LIB]):
        return path
    units = [unit_stem(u) for u in units]
    return link(path, _compile(units, tag, extra_flags) + [obj_path(u) for u in all_units() if u not in units])


def build_jitter(force=False):
    """TEST-ONLY library csrc/libserl_amd_jitter.so: the team kernel families compiled with -DCITW_POISON=1 -DCITW_JITTER=1
    (citation_wave.h: LDS blackboards start as slot-naming signalling NaNs; seeded pseudo-random pauses around every hand-over
    flag and barrier, seed from SERL_JITTER_SEED).  tests/test_gpu_rollout.py runs it against the oracle; the product never loads it."""
    return build_variant(JITTER_LIB, '_jitter', ['-DCITW_POISON=1', '-DCITW_JITTER=1'], TEAM_UNITS, force)


if __name__ == '__main__':
    if '--source-hash' in sys.argv:
        print(source_hash())
        sys.exit(0)
    print(build(force='--force' in sys.argv, verbose=True))
    if '--jitter' in sys.argv:
        print(build_jitter(force='--force' in sys.argv))
