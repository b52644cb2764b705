"""bench.py's contract on the GPU box: the single-GPU line carries every field the driver reads, and
`python bench.py --gpus 2` from a bare shell starts its own two ranks (on a 1-GPU box: both on device 0 over
gloo, labelled as a rehearsal)."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv, **kw):
    """-> the JSON line of `bench.py argv` (and its stderr with stderr=True)."""
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(argv), env=env, text=True,
                       capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return (json.loads(lines[0]), r.stderr) if kw.get('stderr') else json.loads(lines[0])


def test_bench_line_single_gpu():
    out = _bench('--steps', '3', '--warmup', '1', '--full', '--no-cpu-baseline')
    assert out['n_gpus'] == 1 and out['steps'] == 3 and out['warmup'] == 1
    assert out['unit'] == 'M-edges/s' and out['value'] > 0 and out['higher_is_better'] is True
    assert out['scaling'] == 'weak' and out['dtype'] == 'f32' and out['vs_baseline'] is None
    assert abs(out['ms_per_step'] * out['value'] - out['config']['edges_per_rank_step'] / 1e3) < 1e-2 * out['config']['edges_per_rank_step'] / 1e3
    roof = out['roofline']
    assert roof['bound'] == 'hbm' and roof['unit'] == 'GB/s' and roof['peak'] == 8000.0
    assert abs(roof['frac'] - roof['achieved'] / roof['peak']) < 1e-3
    assert 'cached per mesh' in out['config']['workload']
    # the inference configs and the fresh-batch figure ride in the same line
    inf = out['extra']['infer']
    for key, faces in (('configs[1]', 20480), ('configs[3]', 151380)):
        e = inf[key]
        assert 'F=%d' % faces in e['workload'] and e['network_ms'] > 0 and e['M_edges_per_s'] > 0
        k = e['fused_feast_kernel']
        assert k['unit'] == 'GB/s' and abs(k['frac'] - k['achieved'] / 8000.0) < 1e-3
    fb = out['extra']['fresh_batch']
    assert fb['ms_per_step'] > 0 and fb['structure_build_ms_per_mesh'] > 0
    # 4 fresh meshes of the bench size per step: the same edge count as the replayed batch
    assert abs(fb['M_edges_per_s'] * fb['ms_per_step'] - out['config']['edges_per_rank_step'] / 1e3) < 1e-2 * out['config']['edges_per_rank_step'] / 1e3


def _dumped(d):
    import numpy as np
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain run times its steps and reports only them; --dump-outputs writes the last timed step's results, the same
    ones run after run with the same arguments; --steps sets how many steps run after the warm-up."""
    import numpy as np
    out, err = _bench('--steps', '2', '--warmup', '1', '--dump-outputs', str(tmp_path / 'a'), stderr=True)
    assert out['n_gpus'] == 1 and out['steps'] == 2 and out['warmup'] == 1 and out['ms_per_step'] > 0
    assert out['unit'] == 'M-edges/s' and out['value'] > 0 and out['higher_is_better'] is True and out['dtype'] == 'f32'
    assert not {'roofline', 'roofline_mfma', 'extra', 'cpu_baseline'} & set(out)
    assert 'timed 2 steps' in err
    arrays = _dumped(str(tmp_path / 'a'))
    assert set(arrays) == {'pred_vertices', 'pred_normals', 'loss', 'loss_v', 'loss_n', 'grad', 'params'}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays['pred_vertices'].shape == (4 * 10242, 3) and arrays['pred_normals'].shape == (4 * 20480, 3)
    assert arrays['grad'].shape == arrays['params'].shape == (939128,)
    assert abs(float(arrays['loss'][0]) - out['config']['final_loss']) < 1e-5 * max(1.0, abs(out['config']['final_loss']))
    assert abs(float(arrays['loss'][0]) - float(arrays['loss_v'][0] + arrays['loss_n'][0])) < 1e-5
    # same arguments, same inputs: the second process computes the same outputs bit for bit
    _bench('--steps', '2', '--warmup', '1', '--dump-outputs', str(tmp_path / 'b'))
    again = _dumped(str(tmp_path / 'b'))
    assert set(again) == set(arrays) and all(np.array_equal(arrays[k], again[k]) for k in arrays)
    # one more timed step is one more optimiser step; three steps split 2 + 1 (warm-up + timed) end where 1 + 2 did
    more, err = _bench('--steps', '3', '--warmup', '1', '--dump-outputs', str(tmp_path / 'c'), stderr=True)
    assert more['steps'] == 3 and 'timed 3 steps' in err
    assert not np.array_equal(_dumped(str(tmp_path / 'c'))['params'], arrays['params'])
    moved = _bench('--steps', '1', '--warmup', '2', '--dump-outputs', str(tmp_path / 'd'))
    assert moved['steps'] == 1 and np.array_equal(_dumped(str(tmp_path / 'd'))['params'], arrays['params'])


def test_bench_two_ranks_from_a_bare_shell():
    assert torch.cuda.is_available()
    out = _bench('--gpus', '2', '--steps', '3', '--warmup', '1', '--no-roofline', '--no-cpu-baseline')
    assert out['n_gpus'] == 2 and out['config']['parallelism'] == 'dp2'
    assert out['config']['edges_per_rank_step'] == 1351448
    cfg = out['config']
    if torch.cuda.device_count() < 2:
        assert 'rehearsal' in cfg and 'gloo' in cfg['collective'] and cfg['backend'] == 'gloo'
    else:
        assert 'rehearsal' not in cfg and 'nccl' in cfg['collective'] and cfg['backend'] == 'nccl'
    assert cfg['world_size'] == 2 and cfg['collective_us'] > 0
    assert 0 < cfg['rank_ms_per_step']['min'] <= cfg['rank_ms_per_step']['max']
    assert cfg['rank_ms_per_step']['max'] <= out['ms_per_step'] * 1.001


_RCCL_WORKER = r'''
import os, sys, torch
sys.path.insert(0, %(root)r)
import torch.distributed as dist
from geobi_gnn_amd import network
from geobi_gnn_amd.parallel import FlatParameters
os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
dev = torch.device('cuda', 0)
torch.cuda.set_device(dev)
dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
assert dist.get_backend() == 'nccl'
net = network.DualGNN().to(dev)
bucket = FlatParameters(net).bucket
g = torch.Generator().manual_seed(5)
mine = torch.randn(bucket.flat.numel(), generator=g).to(dev)
bucket.flat.copy_(mine)
dist.all_reduce(bucket.flat, op=dist.ReduceOp.SUM)               # what all_reduce_mean issues at N > 1
torch.cuda.synchronize()
assert torch.equal(bucket.flat, mine)
off = bucket.facet_offset(net)
evs = [torch.cuda.Event(), torch.cuda.Event()]
for e in evs:
    e.record()
comm = torch.cuda.Stream(device=dev)
out = bucket.all_reduce_mean_split(off, evs, comm, _single_rank_too=True)     # early collective on the comm stream
torch.cuda.synchronize()
assert torch.equal(out, mine)
dist.barrier()
dist.destroy_process_group()
print('rccl ok')
'''


def test_rccl_single_rank_runs_the_collectives(tmp_path):
    """RCCL itself only runs in the driver's multi-GPU tier; on the one-GPU box the nccl backend is at least brought up on
    a single rank and runs the collectives the data-parallel step issues -- the one-shot all-reduce of the flat bucket and
    the split form with its early collective on a communication stream behind two events."""
    script = tmp_path / 'rccl_worker.py'
    script.write_text(_RCCL_WORKER % {'root': ROOT})
    from helpers import free_port
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(free_port()), HSA_ENABLE_IPC_MODE_LEGACY='0')
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'rccl ok' in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
