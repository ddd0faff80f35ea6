"""Speed of this build against another build of the library (the parent commit's) where a host-side change of
csrc/tower.hip would show: the C2 train step as tools/ab_step.py measures it, and the host microseconds per call of the
launch-bound tiny-batch eager path as tools/host_overhead.py measures them.

The two builds run alternately, each run a fresh child process (ABNET3_HIP_LIB) under its own time limit; the first child
that fails ends the run.  Per figure: the runs, their median and spread ((max - min) / median) per side, and the ratio of
the medians, which passes while it is below 1 + twice the parent's own spread.

python tools/tower_dispatch_ab.py --parent-lib FILE [--runs 5] [--out profiles/tower_dispatch_ab.json]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(script, lib, timeout):
    env = dict(os.environ, ABNET3_HIP_LIB=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', script)], env=env, timeout=timeout, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.stdout.write(r.stdout)
        raise SystemExit('%s with %s exited with %d: nothing more is started' % (script, lib, r.returncode))
    return r.stdout


def step_figures(text):
    return {'c2_step_ms': float(re.search(r'([0-9.]+) ms/step', text).group(1))}


def host_figures(text):
    f = {}
    for name, host in re.findall(r'^(.+?)\s+host\s+([0-9.]+) us/call', text, re.M):
        f['host_us ' + name.strip()] = float(host)
    for name, us in re.findall(r'^C call (\S+)\s+([0-9.]+) us/step', text, re.M):
        f['c_call_us ' + name] = float(us)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', required=True)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--timeout', type=int, default=120, help='seconds per child')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tower_dispatch_ab.json'))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from abnet3_amd import build
    libs = {'parent': os.path.abspath(a.parent_lib), 'this': build.LIB}
    runs = {side: {} for side in libs}
    for i in range(a.runs):
        for script, parse in (('ab_step.py', step_figures), ('host_overhead.py', host_figures)):
            for side in ('parent', 'this') if i % 2 == 0 else ('this', 'parent'):
                for k, v in parse(child(script, libs[side], a.timeout)).items():
                    runs[side].setdefault(k, []).append(v)
        print('run %d of %d done' % (i + 1, a.runs), flush=True)
    res = {'runs_per_side': a.runs, 'bound': 'ratio < 1 + 2 * (max - min) / median of the parent build\'s runs', 'figures': {}}
    ok = True
    for k in runs['parent']:
        p, t = runs['parent'][k], runs['this'][k]
        mp, mt = statistics.median(p), statistics.median(t)
        spread = (max(p) - min(p)) / mp
        fig = {'parent_runs': p, 'this_runs': t, 'parent_median': mp, 'this_median': mt, 'parent_spread': round(spread, 4),
               'this_spread': round((max(t) - min(t)) / mt, 4), 'ratio': round(mt / mp, 4), 'bound': round(1 + 2 * spread, 4)}
        fig['within_bound'] = fig['ratio'] < fig['bound']
        ok = ok and fig['within_bound']
        res['figures'][k] = fig
        print('%-44s parent %9.4f  this %9.4f  ratio %.4f  bound %.4f  %s' % (k, mp, mt, fig['ratio'], fig['bound'],
                                                                               'ok' if fig['within_bound'] else 'SLOWER'), flush=True)
    res['all_within_bound'] = ok
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
