"""Training on folders of OBJ meshes: the loop of code/train_dual.py:100-298 over a dataset.DualDataset, behind the
``train`` command (``python -m geobi_gnn_amd train --data_dir dataset/Synthetic --out_dir log/run1``).

It is the loop of tools/train_synthetic.py with files instead of generated meshes.  A step is: the batch as ONE
disjoint-union graph (data.union_batch_graphs, two launches), every sample of it turned by its own random rotation
(data.rotate_union, one launch per graph: the reference's RandomRotate, applied per sample by its loader), forward,
per-mesh mean losses, backward, Adam over the flat parameter.  Per epoch: evaluation over the test split sample by
sample, best-on-eval checkpoint, schedule, one log line, TensorBoard scalars read back once.

With ``--noise_levels`` the train split needs clean meshes only: its noisy copies are drawn on the device
(dataset.DualDataset(noise=...)), and ``--renoise_every K`` draws them afresh before every K-th epoch.

Single process only.  Not taken over from the reference: the code backup (train_dual.py:131), the ``last_epoch = 500``
of ``--restore``, the ``eval()`` of unknown flags, progress bars.
"""
import argparse
import contextlib
import json
import os
import sys
import time

import torch

from . import meshnoise, network, train_util
from .data import RandomRotate, rotate_union, union_batch_graphs
from .dataset import DualDataset
from .parallel import FlatParameters, add_regularisers, batched_losses, shard_indices

DATA_TYPES = ('Synthetic', 'Kinect_v1', 'Kinect_v2', 'Kinect_Fusion')
TRAIN_TAGS = ('loss_v', 'loss_f', 'dual_loss', 'error_v', 'error_f')
REG_TAGS = (('loss_lap', 'loss_lap_scale'), ('loss_edge', 'loss_edge_scale'))       # a tag of train/ per regulariser that is on
TEST_TAGS = (('loss_v', 'eval_loss_v'), ('loss_f', 'eval_loss_f'), ('error_v', 'eval_error_v'), ('error_f', 'eval_error_f'))


def add_train_flags(parser):
    """The flags of train_dual.py:39-82 that this loop honours, same names and defaults."""
    train_util.add_training_flags(parser)
    parser.add_argument('--data_dir', type=str, required=True,
                        help="the reference's dataset/<data_type> folder: train/ and test/ (each original/ + noisy/), "
                             'optional train_list.txt / test_list.txt')
    parser.add_argument('--data_type', type=str, default='Synthetic', choices=list(DATA_TYPES))
    parser.add_argument('--flag', type=str, default='train', help='free text, kept in the params file')
    parser.add_argument('--seed', type=int, default=None, help='default: drawn, printed and kept in the params file')
    parser.add_argument('--gpu', type=int, default=-1, help='device index (default: the current device)')
    parser.add_argument('--filter_patch_count', type=int, default=100, help='patches of at most this many faces are dropped')
    parser.add_argument('--sub_size', type=int, default=20000, help='faces per patch')
    parser.add_argument('--model_path', type=str, default='', help='initial weights (state dict)')
    parser.add_argument('--out_dir', type=str, required=True)
    parser.add_argument('--rotate', type=str, default='full', choices=['full', 'z', 'none'],
                        help="per-sample random rotation; full = the reference's RandomRotate(False)")
    parser.add_argument('--no_cache', action='store_true', help='neither read nor write <split>/processed_data')
    parser.add_argument('--no_predict', action='store_true', help='do not denoise the test folder after training')
    parser.add_argument('--noise_levels', type=noise_levels_arg, default=None,
                        help='e.g. 0.1,0.2,0.3 (fractions of the mean edge length): draw the noisy copies of the train '
                             'split on the device from <data_dir>/train/original alone; the noise seed is --seed.  The test '
                             'split uses its noisy/ folder if there is one, else it is drawn once')
    parser.add_argument('--noise_kind', type=str, default='gaussian', choices=list(meshnoise.KINDS))
    parser.add_argument('--noise_direction', type=str, default='normal', choices=list(meshnoise.DIRECTIONS))
    parser.add_argument('--noise_fraction', type=float, default=0.3, help='share of the vertices the impulsive kind moves')
    parser.add_argument('--renoise_every', type=int, default=0,
                        help='K > 0: before every epoch with epoch %% K == 0 the train split is drawn afresh (round epoch // K); '
                             '0: the draw-0 noise for the whole run')
    return parser


def noise_levels_arg(text):
    """argparse type of a list of noise levels: '0.1,0.2' -> [0.1, 0.2] (a list, so that it goes into the params file)."""
    return list(meshnoise.parse_levels(text))


def make_rotation(mode, seed):
    """RandomRotate for ``--rotate`` with a generator of its own, seeded: the same seed draws the same matrices."""
    import numpy as np
    if mode == 'none':
        return None
    return RandomRotate(z_rotated=mode == 'z', rng=np.random.default_rng(seed))


def reg_scales(opt):
    """(--loss_lap_scale, --loss_edge_scale); options from before the flags existed have neither: 0."""
    return tuple(float(getattr(opt, flag, 0) or 0) for _, flag in REG_TAGS)


def train_tags(opt):
    """The scalars train_epoch hands out per step: TRAIN_TAGS, then the tag of every regulariser whose scale is not 0."""
    return TRAIN_TAGS + tuple(tag for (tag, _), scale in zip(REG_TAGS, reg_scales(opt)) if scale != 0)


def loss_sampling(opt, epoch, batch):
    """What ``--loss_v SCD`` draws in a step, as parallel.batched_losses takes it (None for every other loss): seed =
    opt.seed, draw = the epoch, the stream of a mesh = its index in the dataset -- a mesh's points depend on (seed, epoch,
    which mesh) and never on the batch it lands in.  Options from before the flag existed: 10 000 points."""
    if opt.loss_v != 'SCD':
        return None
    return dict(n=int(getattr(opt, 'loss_samples', 10000)), seed=int(opt.seed), draw=int(epoch),
                stream_ids=[int(i) for i in batch])


def train_epoch(net, flat, optimizer, samples, opt, epoch, rotate=None, scalars=None, iteration=0):
    """One pass over ``samples`` (a DualDataset or a list of resident pairs) in parallel.shard_indices order (seed,
    epoch), ``opt.batch_size`` samples per step; the last, short batch still steps.  scalars: optional list that takes
    (iteration, device tensor of the train_tags(opt) values: the five TRAIN_TAGS, then the unscaled term of every
    regulariser that is on) per step -- nothing is read back here.  A regulariser (``opt.loss_lap_scale``,
    ``opt.loss_edge_scale``) whose scale is 0 is not computed.  ``opt.loss_v == 'SCD'`` draws as loss_sampling says.
    -> (iteration, loss of the last step as a device scalar)"""
    net.train()
    order = shard_indices(len(samples), 0, 1, seed=opt.seed, epoch=epoch)
    lap_scale, edge_scale = reg_scales(opt)
    loss = None
    for s in range(0, len(order), opt.batch_size):
        batch = order[s:s + opt.batch_size]
        dv, df = union_batch_graphs([samples[i] for i in batch])        # always a copy: the samples are never written
        if rotate is not None:
            rotate_union(dv, df, rotate.matrices(len(batch)))
        flat.bucket.zero()
        vp, npred, _ = net((dv.shallow_copy(), df.shallow_copy()))
        lv, ln = batched_losses(vp, npred, dv, df, opt.loss_v, opt.loss_n, sampling=loss_sampling(opt, epoch, batch))
        loss = network.dual_loss(lv, ln, opt.loss_v_scale, opt.loss_n_scale)
        loss, regs = add_regularisers(loss, vp, dv, lap_scale, edge_scale)
        loss.backward()
        optimizer.step()
        iteration += len(batch)
        if scalars is not None:
            with torch.no_grad():
                scalars.append((iteration, torch.stack([lv.detach(), ln.detach(), loss.detach(),
                                                        network.error_v(vp.detach(), dv.y),
                                                        network.error_n(npred.detach(), df.y)] + regs)))
    return iteration, loss


def evaluate(net, samples, opt):
    """train_dual.py:233-259: node-count-weighted means over the samples, one by one.
    -> dict(eval_loss_v, eval_loss_f, eval_error_v, eval_error_f)"""
    net.eval()
    meter = train_util.EvalMeter()
    with torch.no_grad():
        for i in range(len(samples)):
            a, b = samples[i]
            vp, npred, _ = net((a.shallow_copy(), b.shallow_copy()))
            meter.add_prediction(vp, npred, a, b, opt.loss_v, opt.loss_n, samples=int(getattr(opt, 'loss_samples', 10000)),
                                 seed=int(opt.seed or 0))
    return meter.result()


class _Tee(object):
    def __init__(self, stream, path):
        self.stream, self.file = stream, open(path, 'w')

    def write(self, text):
        self.stream.write(text)
        self.file.write(text)

    def flush(self):
        self.stream.flush()
        self.file.flush()


def require_single_process():
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise SystemExit('geobi_gnn_amd train runs in a single process (WORLD_SIZE = %s): the data-parallel loop is '
                         'tools/train_synthetic.py' % os.environ['WORLD_SIZE'])


def require_known_losses(opt):
    """``--loss_v`` / ``--loss_n`` are free text to the parser (as in train_dual.py:57-58): a wrong name ends the command
    here, before the device is touched or a mesh is read, with the valid names in the message."""
    try:
        network.check_loss_names(opt.loss_v, opt.loss_n)
    except ValueError as e:
        raise SystemExit('geobi_gnn_amd train: %s' % e)


def train(opt, dev, predict=None):
    """The ``train`` command on device ``dev``.  Writes into ``opt.out_dir``: GeoBi-GNN_<data_type>_model.pth (best state dict, the
    reference's keys), GeoBi-GNN_<data_type>_params.json (the options), training_info.txt (what was printed), train/ and
    test/ event files and -- through ``predict`` (the ``denoise`` command's function) unless ``opt.no_predict`` --
    result/ with the denoised test meshes (train_dual.py:297-298).  -> exit status"""
    require_single_process()
    require_known_losses(opt)
    if opt.seed is None:
        import random
        opt.seed = random.randint(1, 10000)
    opt.force_depth = opt.data_type in ('Kinect_v1', 'Kinect_v2')          # train_dual.py:93-94
    opt.pool_type = 'max'
    os.makedirs(opt.out_dir, exist_ok=True)
    name = 'GeoBi-GNN_%s' % opt.data_type
    model_file = os.path.join(opt.out_dir, name + '_model.pth')
    tee = _Tee(sys.stdout, os.path.join(opt.out_dir, 'training_info.txt'))
    with contextlib.redirect_stdout(tee):
        try:
            return _train(opt, dev, name, model_file, predict)
        finally:
            tee.flush()
            tee.file.close()


def _train(opt, dev, name, model_file, predict):
    print('Training flag: %s_%s' % (name, opt.flag))
    print('Random seed: %d\n' % opt.seed)
    torch.manual_seed(opt.seed)
    options = {k: v for k, v in sorted(vars(opt).items()) if isinstance(v, (int, float, str, bool, list, type(None)))}
    with open(os.path.join(opt.out_dir, name + '_params.json'), 'w') as fh:
        json.dump(options, fh, indent=1)
    print(json.dumps(options), flush=True)

    noise = None
    if getattr(opt, 'noise_levels', None):
        noise = meshnoise.NoiseOptions(opt.noise_levels, opt.noise_kind, opt.noise_direction, opt.noise_fraction, opt.seed)
    renoise_every = int(getattr(opt, 'renoise_every', 0) or 0)
    if renoise_every < 0 or (renoise_every and noise is None):
        raise SystemExit('geobi_gnn_amd train: --renoise_every needs --noise_levels and K >= 0')

    def split(which):
        lst = which + '_list.txt'
        t0 = time.time()
        # the test split keeps its noise files where it has some: only a split without noisy/ is drawn (once, round 0)
        drawn = noise if which == 'train' or not os.path.isdir(os.path.join(opt.data_dir, which, 'noisy')) else None
        ds = DualDataset(opt.data_dir, which, lst if os.path.isfile(os.path.join(opt.data_dir, lst)) else None,
                         submesh_size=opt.sub_size, filter_patch_count=opt.filter_patch_count, data_type=opt.data_type,
                         device=dev, cache=not opt.no_cache, noise=drawn)
        print('%s: %d samples from %d files (%d skipped) in %.2f s' % (which, len(ds), len(ds.pairs), ds.skipped,
                                                                      time.time() - t0), flush=True)
        return ds
    train_set, test_set = split('train'), split('test')

    net = network.DualGNN(force_depth=opt.force_depth, pool_type=opt.pool_type, wei_param=opt.wei_param)
    if opt.model_path:
        net.load_state_dict(torch.load(opt.model_path, map_location='cpu', weights_only=True))
    net = net.to(dev)
    flat = FlatParameters(net)
    optimizer = train_util.make_optimizer(opt, flat.parameters(), fused=True if opt.optimizer == 'adam' else None)
    sch = train_util.make_scheduler(opt, optimizer)
    ckpt = train_util.BestCheckpoint(model_file)
    rotate = make_rotation(opt.rotate, opt.seed)
    train_writer = train_util.SummaryWriter(os.path.join(opt.out_dir, 'train'))
    test_writer = train_util.SummaryWriter(os.path.join(opt.out_dir, 'test'))
    test_writer.add_text('train_params', json.dumps(options))

    # the net as initialised, before any step: what the best evaluation error is measured against
    res = evaluate(net, test_set, opt)
    print(json.dumps({'epoch': 0, 'eval_loss_v': res['eval_loss_v'], 'eval_loss_f': res['eval_loss_f'],
                      'eval_error_v': res['eval_error_v'], 'eval_error_f_deg': res['eval_error_f']}), flush=True)
    iteration = 0
    for epoch in range(1, opt.max_epoch + 1):
        t0 = time.time()
        scalars = []
        if renoise_every > 0 and epoch % renoise_every == 0:
            train_set.resample(epoch // renoise_every)
        iteration, loss = train_epoch(net, flat, optimizer, train_set, opt, epoch, rotate, scalars, iteration)
        # the reference reads five scalars back per iteration (.item()); here they stay on the device until the epoch ends
        for (it, _), vals in zip(scalars, torch.stack([v for _, v in scalars]).tolist() if scalars else []):
            for tag, v in zip(train_tags(opt), vals):
                train_writer.add_scalar(tag, v, it)
        train_writer.flush()
        res = evaluate(net, test_set, opt)
        rec = {'epoch': epoch, 'train_loss': float(loss.detach()), 'eval_loss_v': res['eval_loss_v'],
               'eval_loss_f': res['eval_loss_f'], 'eval_error_v': res['eval_error_v'],
               'eval_error_f_deg': res['eval_error_f'], 'lr': optimizer.param_groups[0]['lr'],
               'epoch_s': round(time.time() - t0, 3)}
        rec['saved'] = ckpt.update(net, rec['eval_error_f_deg'])          # keys: gnn_v.l_conv1.lin.weight ... fc_f2.bias
        print(json.dumps(rec), flush=True)
        for tag, key in TEST_TAGS:
            test_writer.add_scalar(tag, res[key], iteration)
        test_writer.flush()
        train_util.step_scheduler(opt, sch, rec['eval_error_f_deg'])
    train_writer.close()
    test_writer.close()
    print('\n%s_%s\nbest error: %s' % (name, opt.flag, ckpt.best), flush=True)
    if predict is None or opt.no_predict:
        return 0
    if not os.path.exists(model_file):
        print('no model was saved (the evaluation error was never finite): nothing to predict with', file=sys.stderr)
        return 1
    noisy_dir = ''
    if test_set.noise is not None:
        # the inputs of result/: the round-0 test meshes the evaluation ran on, as files a user can look at
        noisy_dir = os.path.join(opt.out_dir, 'test_noisy')
        test_set.write_noisy(noisy_dir)
    return predict(argparse.Namespace(model=model_file, data_dir=os.path.join(opt.data_dir, 'test'), noisy_dir=noisy_dir,
                                      out_dir=os.path.join(opt.out_dir, 'result'), sub_size=opt.sub_size, n_iter=60,
                                      data_type=opt.data_type, wei_param=opt.wei_param, force_depth=opt.force_depth,
                                      pool_type=opt.pool_type, gpu=opt.gpu))
