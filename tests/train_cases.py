"""What the device tests of training, noise and filtering share: OBJ splits written from icospheres, training options,
one epoch of the package loop, the package's command line as a child process, and the bit-for-bit comparison of two
dataset samples."""
import argparse
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_split(root, split, names, freq, sigmas, seed0):
    """original/NAME.obj + noisy/NAME_n<k>.obj per sigma -> {sample name: (noisy file, original file)}"""
    from geobi_gnn_amd import meshgen, meshio
    files = {}
    for sub in ('original', 'noisy'):
        os.makedirs(os.path.join(root, split, sub), exist_ok=True)
    for i, name in enumerate(names):
        original = os.path.join(root, split, 'original', name + '.obj')
        for k, sigma in enumerate(sigmas, 1):
            noisy, clean, faces = meshgen.noisy_icosphere(freq, sigma, seed=seed0 + 10 * i + k)
            noisy_file = os.path.join(root, split, 'noisy', '%s_n%d.obj' % (name, k))
            meshio.write_obj(noisy_file, noisy, faces)
            files['%s_n%d' % (name, k)] = (noisy_file, original)
        meshio.write_obj(original, clean, faces)
    return files


def _csr(d):
    g = d.graph()
    return g.rowptr_out, g.col_out, g.weights_sorted(d.edge_weight)


def _assert_same_sample(got, want, edge_weight_as_stored=True):
    for a, b in zip(got, want):
        assert torch.equal(a.x, b.x) and torch.equal(a.y, b.y)
        for s, t in zip(_csr(a), _csr(b)):
            assert torch.equal(s, t)
        if edge_weight_as_stored:
            assert torch.equal(a.edge_weight, b.edge_weight)
        da, db = getattr(a, 'depth_direction', None), getattr(b, 'depth_direction', None)
        assert (da is None) == (db is None) and (da is None or torch.equal(da, db))
    assert torch.equal(got[1].fv_indices, want[1].fv_indices)


def _options(**kw):
    from geobi_gnn_amd import train_util
    opt = train_util.add_training_flags(argparse.ArgumentParser()).parse_args([])
    opt.seed = 7
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


def _epoch(samples, dev, opt, rotate=None, epochs=1):
    """Flat parameters after `epochs` passes of trainer.train_epoch from a seed-initialised net."""
    from geobi_gnn_amd import network, train_util, trainer
    from geobi_gnn_amd.parallel import FlatParameters
    torch.manual_seed(11)
    net = network.DualGNN().to(dev)
    flat = FlatParameters(net)
    optimizer = train_util.make_optimizer(opt, flat.parameters(), fused=True)
    for epoch in range(1, epochs + 1):
        trainer.train_epoch(net, flat, optimizer, samples, opt, epoch, rotate=rotate)
    torch.cuda.synchronize()
    return flat.flat_param.detach().clone()


def _run(args, timeout=600):
    """python -m geobi_gnn_amd ARGS as one child process"""
    run = subprocess.run([sys.executable, '-m', 'geobi_gnn_amd'] + list(args), cwd=ROOT, timeout=timeout, capture_output=True,
                         text=True)                                     # a cold `import torch` alone can take a minute
    print(run.stdout)
    print(run.stderr)
    return run


def _train_command(data_dir, out_dir, extra=()):
    return _run(['train', '--data_dir', data_dir, '--out_dir', out_dir, '--max_epoch', '5', '--batch_size', '2', '--seed', '31']
                + list(extra))
