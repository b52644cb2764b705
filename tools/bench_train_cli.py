"""Epoch time of `python -m geobi_gnn_amd train` on files against tools/train_synthetic.py on generated meshes of the
same sizes, alternated as child processes; dataset build / cache-load time per mesh from the command's own log.

  python tools/bench_train_cli.py [--freq 32] [--pairs 5] [--epochs 4] [--work DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geobi_gnn_amd import meshgen, meshio          # noqa: E402


def write_split(root, split, names, freq, sigmas, seed0):
    for sub in ('original', 'noisy'):
        os.makedirs(os.path.join(root, split, sub), exist_ok=True)
    for i, name in enumerate(names):
        for k, sigma in enumerate(sigmas, 1):
            noisy, clean, faces = meshgen.noisy_icosphere(freq, sigma, seed=seed0 + 10 * i + k)
            meshio.write_obj(os.path.join(root, split, 'noisy', '%s_n%d.obj' % (name, k)), noisy, faces)
        meshio.write_obj(os.path.join(root, split, 'original', name + '.obj'), clean, faces)


def run(cmd):
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit('child failed (%d): %s' % (r.returncode, ' '.join(cmd)))
    return r.stdout


def epochs_of(stdout):
    recs = []
    for ln in stdout.splitlines():
        if ln.startswith('{"epoch"'):
            rec = json.loads(ln)
            if rec['epoch'] >= 1:
                recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--freq', type=int, default=32)
    ap.add_argument('--pairs', type=int, default=5)
    ap.add_argument('--epochs', type=int, default=4)
    ap.add_argument('--work', type=str, default='')
    opt = ap.parse_args()
    work = opt.work or tempfile.mkdtemp(prefix='geobi_train_cli_')
    data = os.path.join(work, 'Synthetic')
    write_split(data, 'train', ('a', 'b', 'c', 'd'), opt.freq, (0.1, 0.2, 0.3), 1000)      # 12 files
    write_split(data, 'test', ('t', 'u'), opt.freq, (0.1, 0.3), 5000)                     # 4 files
    py = sys.executable
    common = ['--batch_size', '4', '--max_epoch', str(opt.epochs)]
    forms = {
        'train --rotate none': lambda k: [py, '-m', 'geobi_gnn_amd', 'train', '--data_dir', data, '--out_dir',
                                          os.path.join(work, 'none%d' % k), '--seed', '1', '--rotate', 'none', '--no_predict'] + common,
        'train --rotate full': lambda k: [py, '-m', 'geobi_gnn_amd', 'train', '--data_dir', data, '--out_dir',
                                          os.path.join(work, 'full%d' % k), '--seed', '1', '--rotate', 'full', '--no_predict'] + common,
        'tools/train_synthetic.py': lambda k: [py, os.path.join(ROOT, 'tools', 'train_synthetic.py'), '--freq', str(opt.freq),
                                               '--n_train', '12', '--n_eval', '4'] + common,
    }
    times = {k: [] for k in forms}
    info = []
    for k in range(opt.pairs):
        for name, cmd in forms.items():
            out = run(cmd(k))
            recs = epochs_of(out)
            times[name].append(min(r['epoch_s'] for r in recs[1:]))       # the first epoch builds caches and arenas
            info += [name + ' | ' + ln for ln in out.splitlines() if ln.startswith(('train:', 'test:'))]
            if k == 0:
                print('%s: eval normal error per epoch %s' % (name, [round(r['eval_error_f_deg'], 4) for r in recs]), flush=True)
    print('epoch time (s; best of epochs 2..%d of each run; %d alternated runs; 12 meshes of %d faces, batch 4, 4 evaluation meshes)'
          % (opt.epochs, opt.pairs, 20 * opt.freq ** 2))
    for name, t in times.items():
        print('  %-26s median %.3f  min %.3f  max %.3f  all %s' % (name, float(np.median(t)), min(t), max(t), t))
    print('dataset construction as the command logged it (first run: built and cached; later runs: loaded from processed_data/)')
    for ln in info:
        print('  ' + ln)


if __name__ == '__main__':
    main()
