"""Command line of the package: train on folders of OBJ meshes, denoise a folder, score a folder of results.

  python -m geobi_gnn_amd train --data_dir dataset/Synthetic --out_dir log/run1 [--batch_size 4] [--max_epoch 100]
  python -m geobi_gnn_amd denoise --model net.pt --data_dir DIR [--out_dir DIR/result] [--sub_size 20000]
  python -m geobi_gnn_amd denoise --method bnf --data_dir DIR [--normal_iters 20] [--sigma_r 0.35] [--sigma_s 1.0] [--n_iter 20]
  python -m geobi_gnn_amd denoise --method gnf --data_dir DIR [the same flags]
  python -m geobi_gnn_amd eval --result_dir DIR/result --original_dir DIR/original [--align [--scale]] [--free] [--index grid]
  python -m geobi_gnn_amd align --data_dir DIR --target_dir DIR2 [--out_dir DIR/aligned] [--scale] [--reflect] [--max_iter 100]
  python -m geobi_gnn_amd noise --data_dir DIR [--levels 0.1,0.2,0.3] [--kind gaussian] [--direction normal] [--seed 1]
  python -m geobi_gnn_amd clean --data_dir DIR [--out_dir DIR/clean] [--weld_tol 0] [--no_weld] [--no_manifold]
  python -m geobi_gnn_amd denoise ... --clean [--weld_tol 0] [--no_weld] [--no_manifold] [--orient] [--min_component N]
  python -m geobi_gnn_amd clean ... [--orient] [--min_component N] [--drop_intersecting] [--outward]
  python -m geobi_gnn_amd info --data_dir DIR [--weld_tol 0] [--no_weld] [--intersections] [--solid] [--gpu -1]
  python -m geobi_gnn_amd sample --data_dir DIR [--out_dir DIR/samples] --n N [--seed 1] [--normals] [--gpu -1]
  python -m geobi_gnn_amd eval ... --free --samples N [--seed 1]
  python -m geobi_gnn_amd eval ... --free --signed
  python -m geobi_gnn_amd align ... --samples N [--seed 1]
  python -m geobi_gnn_amd subdivide --data_dir DIR [--out_dir DIR/subdivided] [--levels 1] [--scheme midpoint|loop]
  python -m geobi_gnn_amd subdivide --data_dir DIR (--max_edge L | --max_edge_diag R) [--max_rounds 16]
  python -m geobi_gnn_amd decimate --data_dir DIR [--out_dir DIR/decimated] (--ratio R | --faces N) [--max_cost C] [--max_rounds 256]
  python -m geobi_gnn_amd remesh --data_dir DIR [--out_dir DIR/remeshed] [--target_edge L | --target_edge_diag R] [--iterations 5]
                                 [--feature_angle 40] [--relax_lambda 0.5] [--max_rounds 64] [--project [--index grid]]
  python -m geobi_gnn_amd project --data_dir DIR --target_dir DIR2 [--out_dir DIR/projected] [--max_dist D | --max_dist_diag R]
                                  [--index grid]
  python -m geobi_gnn_amd fill --data_dir DIR [--out_dir DIR/filled] [--max_hole_edges N] [--gpu -1]

`denoise` is predict_dir of the reference (code/test_dual.py:25-150): with DIR/original and DIR/noisy
present, every original/NAME.obj is paired with its noisy/NAME_n*.obj and the two angular errors are printed per file
and as face-weighted means; otherwise every DIR/*.obj is denoised without ground truth.  `--method bnf` needs no model: it
runs the bilateral normal filter (filters.py) on the same files and writes the same outputs -- the baseline row; `--method
gnf` is the guided normal filter, the model-free method for high noise, through the same loop and flags.  `eval` is
data_util.eval_denoising_result (code/data_util.py:559-638).  `train` is code/train_dual.py:100-298 (trainer.py): DIR holds
train/ and test/, each with original/ and noisy/; the best model, the options, the log, TensorBoard event files and the
denoised test meshes go to --out_dir.  `noise` has no counterpart in the reference (its dataset is a download): it writes
DIR/noisy/NAME_n<k>.obj for every DIR/original/NAME.obj, the layout `train` and `denoise` read.  `clean` (meshclean.py)
repairs files that are no clean triangle meshes -- welds vertices, drops degenerate faces and faces that would give a
directed edge a second owner, drops unused vertices -- which openmesh does for the reference while it reads a file; with
DIR/original present the cleaning is computed from original/NAME.obj and the SAME maps are applied to every
noisy/NAME_n*.obj of equal size (welding noisy coordinates would be wrong: duplicates carry independent noise).  `denoise
--clean` cleans every file before it is denoised and writes the result in the file's own numbering.  `--orient` (meshtopo.py)
winds the faces of every connected part consistently before the half-edge rule, which otherwise drops one of every two
neighbours wound in opposite senses; `--min_component N` drops the edge-connected parts of fewer than N faces (scan debris).
`info` prints what a file is before any of that is chosen: edges, boundary, complex and inconsistent edges, parts, whether
it is closed and orientable; `info --intersections` (meshselfx.py) also says whether the surface passes through itself:
the pairs of faces that intersect, the faces in such a pair, the pairs folded flat onto each other.  `clean
--drop_intersecting` drops those faces, and `fill` closes what that opens.  `align` (ops.icp) brings every DIR/NAME_*.obj -- or DIR/NAME.obj where a stem has none -- into
the frame of DIR2/NAME.obj by rigid point-to-point ICP and writes it with its own faces; the two meshes may differ in size.
`eval --align` does the same before it scores (AlignInfo.txt beside ErrorInfo_h.txt), `eval --free` scores pairs whose
vertex counts or face tables differ (ErrorInfo_free.txt).  `sample` (meshsample.py) writes N points drawn uniformly by
area on the surface of every DIR/original/*.obj (or DIR/*.obj) as OUT/NAME.obj with `v` lines only (`--normals`: a `vn`
line per point); `eval --free --samples N` also scores from such points of both surfaces (ErrorInfo_sampled.txt beside
an unchanged ErrorInfo_free.txt), `align --samples N` aligns to the target's vertices followed by N points of its
surface -- what a CAD target of a few large triangles needs.  `subdivide` (meshsubdiv.py) makes every mesh denser:
`--levels K` passes that split every edge (at its midpoint, or with `--scheme loop` by Loop's masks), or `--max_edge L` /
`--max_edge_diag R` (L = R times the diagonal of the mesh's bounding box) rounds that split only the edges longer than L;
with DIR/original present the refinement is planned on original/NAME.obj and applied to every noisy/NAME_n*.obj of equal
size, which keeps the pairs in correspondence.  `decimate` (meshdecim.py) is its inverse: rounds of quadric edge collapses
until `--faces N` or `--ratio R` times the faces are left (`--max_cost C`: no collapse dearer than C), boundaries kept at
full resolution, with the same folders and the same pairing of noisy files.  `fill` (meshfill.py) closes the holes of every
mesh: each closed boundary loop (`--max_hole_edges N`: of at most N edges, which leaves an open border open) gets one new
vertex at the mean of its rim and a fan of faces, with the same folders; a noisy file gets its original's fill with every
new vertex at the mean of its own rim.  `remesh --project` (meshproject.py) ends every iteration by moving the relaxed
vertices back to their closest points on the input surface, so the result does not drift off it, and every output vertex
keeps a (face, barycentric) address on the input: with DIR/noisy present its files are carried along through that map.
`project` moves the vertices of every DIR/NAME_*.obj -- or DIR/NAME.obj -- to their closest points on the surface of
DIR2/NAME.obj (the pairing of `align`) and writes it with its own faces; `--max_dist D` / `--max_dist_diag R` (R times the
diagonal of the target's bounding box) leaves the vertices that are farther away where they are.  All device work runs in
this one process.
"""
import argparse
import os
import sys
import time

import numpy as np

from . import folders


BNF_N_ITER = 20          # vertex-update sweeps of --method bnf / gnf when --n_iter is not given (filters.bilateral_denoise's default)


class _StoreGiven(argparse.Action):
    """store, and note in <dest>_given that the flag was on the command line"""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        setattr(namespace, self.dest + '_given', True)


def _denoise_list(data_dir, noisy_dir=''):
    """[(noisy file, ground-truth file or None)] in sorted order.  noisy_dir: where the NAME_n*.obj of DIR/original are,
    if not in DIR/noisy (`train` hands over the test meshes it drew itself)."""
    original_dir, noisy_dir = os.path.join(data_dir, 'original'), noisy_dir or os.path.join(data_dir, 'noisy')
    if os.path.isdir(original_dir) and os.path.isdir(noisy_dir):
        return [(noisy, gt) for gt in folders.obj_files(original_dir)
                for noisy in folders.noisy_of(noisy_dir, folders.stem_of(gt))]
    return [(f, None) for f in folders.obj_files(data_dir)]


def _device(gpu):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('geobi_gnn_amd: no GPU visible -- this path runs on the MI355X only (there is no CPU fallback)')
    dev = torch.device('cuda:%d' % gpu if gpu >= 0 else 'cuda:%d' % torch.cuda.current_device())
    torch.cuda.set_device(dev)
    return dev


def denoise(opt):
    import torch
    from . import meshio
    from ._lib import GeobiError
    # `train` hands over its own options, which have none of the filter's flags: read them with their defaults
    method = getattr(opt, 'method', 'gnn')
    # --n_iter keeps its default of 60; the filter takes 20 sweeps unless the flag was given
    n_iter = opt.n_iter if method == 'gnn' or getattr(opt, 'n_iter_given', False) else BNF_N_ITER
    dev = _device(opt.gpu)
    jobs = _denoise_list(opt.data_dir, getattr(opt, 'noisy_dir', ''))
    out_dir = opt.out_dir or os.path.join(opt.data_dir, 'result')
    os.makedirs(out_dir, exist_ok=True)
    if method in ('bnf', 'gnf'):
        from . import filters
        filter_fn = filters.bilateral_denoise if method == 'bnf' else filters.guided_denoise
        normal_iters, sigma_r, sigma_s = (getattr(opt, 'normal_iters', 20), getattr(opt, 'sigma_r', 0.35),
                                          getattr(opt, 'sigma_s', 1.0))
        print('\n%s normal filter, normal_iters:%d, sigma_r:%g, sigma_s:%g, %d files ...\n'
              % ('Bilateral' if method == 'bnf' else 'Guided', normal_iters, sigma_r, sigma_s, len(jobs)), flush=True)

        def run(points, faces, gt_points):
            return filter_fn(points, faces, normal_iters=normal_iters, sigma_r=sigma_r, sigma_s=sigma_s, n_iter=n_iter,
                             data_type=opt.data_type, gt_points=gt_points, device=dev)
    else:
        from . import network, patches
        torch.manual_seed(0)
        net = network.DualGNN(force_depth=opt.force_depth, pool_type=opt.pool_type, wei_param=opt.wei_param)
        if opt.model:
            net.load_state_dict(torch.load(opt.model, map_location='cpu', weights_only=True))
        net = net.to(dev).eval()
        print('\nInfer %s, sub_size:%d, %d files ...\n' % (opt.model or 'random init', opt.sub_size, len(jobs)), flush=True)

        def run(points, faces, gt_points):
            return patches.predict_mesh(net, points, faces, sub_size=opt.sub_size, n_iter=n_iter,
                                        data_type=opt.data_type, gt_points=gt_points, distributed=False)
    clean = getattr(opt, 'clean', False)
    if clean:
        from . import meshclean
    done, failed = [], 0
    for noisy_file, gt_file in jobs:
        t0 = time.time()
        try:
            points, faces = meshio.read_obj(noisy_file)
            if faces.shape[0] == 0:
                raise ValueError('%s: no faces' % noisy_file)
            loose = 0 if clean else meshio.unreferenced_vertices(points.shape[0], faces)
            if loose:
                raise ValueError('%s: %d of %d vertices are referenced by no face (the vertex update averages over a '
                                 "vertex's faces)" % (noisy_file, loose, points.shape[0]))
            gt_points = None
            if gt_file is not None:
                gt_points, gt_faces = meshio.read_obj(gt_file)
                if gt_points.shape != points.shape or gt_faces.shape != faces.shape:
                    raise ValueError('%s (V = %d, F = %d) and its ground truth %s (V = %d, F = %d) differ in size'
                                     % (noisy_file, points.shape[0], faces.shape[0], gt_file, gt_points.shape[0],
                                        gt_faces.shape[0]))
            if clean:
                # the cleaning comes from the file itself; the ground truth follows its maps, the result goes back to the
                # file's numbering and faces (welded duplicates share one position, unused vertices keep theirs)
                cleaned = meshclean.clean_mesh(points, faces, weld_tol=_weld_tol(opt), manifold=not opt.no_manifold, device=dev,
                                               **_topo_args(opt))
                n_faces = cleaned.faces.shape[0]
                if n_faces == 0:
                    raise ValueError('%s: no faces left after cleaning' % noisy_file)
                if gt_points is not None:
                    gt_points = meshclean.apply(cleaned, gt_points)
                with torch.no_grad():
                    r = run(cleaned.points.cpu().numpy(), cleaned.faces.cpu().numpy(), gt_points)
                updated = meshclean.scatter_back(cleaned, r['V_updated'].to(dev), torch.from_numpy(points).to(dev))
            else:
                n_faces = faces.shape[0]
                with torch.no_grad():
                    r = run(points, faces, gt_points)
                updated = r['V_updated']
            rst_file = os.path.join(out_dir, '%s-%d.obj' % (os.path.basename(noisy_file)[:-4], n_iter))
            meshio.write_obj(rst_file, updated.cpu().numpy(), faces)
        except (ValueError, OSError, GeobiError) as e:
            failed += 1
            print('skipped: %s' % e, file=sys.stderr, flush=True)
            continue
        angle1, angle2 = (r['angle1'], r['angle2']) if gt_file is not None else (0.0, 0.0)
        done.append((n_faces, angle1, angle2))
        print("angle1: %9.6f,  angle2: %9.6f,  faces: %6d,  time: %7.4f s,  '%s'"
              % (angle1, angle2, n_faces, time.time() - t0, os.path.basename(rst_file)), flush=True)
    if done:
        err = np.asarray(done, dtype=np.float64).T
        count = err[0].sum()
        print('\nNum_face: %6d,  angle_mean1: %.6f,  angle_mean2: %.6f'
              % (count, (err[0] * err[1]).sum() / count, (err[0] * err[2]).sum() / count))
    print('\n--- end ---')
    if failed:
        print('%d of %d files skipped' % (failed, len(jobs)), file=sys.stderr)
    return 1 if failed or not jobs else 0


def _index_of(opt):
    """--index none|grid -> the index= keyword of the searches' callers"""
    return None if opt.index == 'none' else opt.index


def evaluate(opt):
    from . import mesheval
    from ._lib import GeobiError
    dev = _device(opt.gpu)
    stats = {}
    t0 = time.time()
    try:
        more = {'signed': True} if opt.signed else {}
        rows, _ = mesheval.eval_dirs(opt.result_dir, opt.original_dir, device=dev, stats=stats, align=opt.align, free=opt.free,
                                     estimate_scale=opt.scale, samples=opt.samples, seed=opt.seed, index=_index_of(opt), **more)
    except (ValueError, OSError, GeobiError) as e:
        print('eval failed: %s' % e, file=sys.stderr)
        return 1
    print('%d pairs in %.3f s (reading OBJ %.3f s, device work %.3f s)'
          % (len(rows), time.time() - t0, stats.get('parse', 0.0), stats.get('device', 0.0)))
    return 0 if rows else 1


def align_list(data_dir, target_dir):
    """[(source file, target file)] in sorted order: mesheval.pair_files' pairing, every target_dir/NAME.obj with every
    data_dir/NAME_*.obj, and with data_dir/NAME.obj where the stem has no NAME_*.obj."""
    jobs = []
    for target in folders.obj_files(target_dir):
        stem = folders.stem_of(target)
        found = folders.variants_of(data_dir, stem)
        same = os.path.join(data_dir, stem + '.obj')
        if not found and os.path.isfile(same):
            found = [same]
        jobs.extend((f, target) for f in found)
    return jobs


def align(opt):
    """Every source mesh of --data_dir aligned to its target of --target_dir by rigid ICP on the device (mesheval.align),
    written to --out_dir with aligned vertices and its own faces."""
    from . import mesheval, meshio, meshnoise
    dev = _device(opt.gpu)
    jobs = align_list(opt.data_dir, opt.target_dir)
    out_dir = opt.out_dir or os.path.join(opt.data_dir, 'aligned')
    os.makedirs(out_dir, exist_ok=True)
    print('\nAlign, scale %s, reflections %s, max_iter %d, rmse_thr %g, %d files ...\n'
          % ('on' if opt.scale else 'off', 'on' if opt.reflect else 'off', opt.max_iter, opt.rmse_thr, len(jobs)), flush=True)

    def one(job, skip):
        source, target = job
        t0 = time.time()
        points, faces = meshio.read_obj(source)
        t_points, t_faces = meshio.read_obj(target)
        if points.shape[0] == 0 or t_points.shape[0] == 0:
            raise ValueError('%s or its target %s has no vertices' % (source, target))
        sampling = {}
        if opt.samples:         # the target's surface joins its vertices: the stream is the target's name
            sampling = {'target_faces': t_faces, 'samples': opt.samples, 'seed': opt.seed,
                        'stream_id': meshnoise.stream_of(folders.stem_of(target))}
        res = mesheval.align(points, t_points, device=dev, estimate_scale=opt.scale, allow_reflection=opt.reflect,
                             max_iterations=opt.max_iter, relative_rmse_thr=opt.rmse_thr, **sampling)
        out_file = os.path.join(out_dir, os.path.basename(source))
        meshio.write_obj(out_file, res.xt.cpu().numpy(), faces)
        info = mesheval.align_info(res)
        print("iterations: %3d,  converged: %s,  rmse: %.6e,  scale: %.6f,  angle: %10.6f,  shift: %.6f,  time: %7.4f s,  '%s'"
              % (info['icp_iterations'], 'yes' if info['icp_converged'] else 'no', info['icp_rmse'], info['icp_scale'],
                 info['icp_angle'], info['icp_shift'], time.time() - t0, os.path.basename(out_file)), flush=True)

    return folders.walk(jobs, one)


def noise(opt):
    """original/NAME.obj -> noisy/NAME_n<k>.obj for every level k = 1.., drawn on the device (meshnoise)."""
    from . import meshio, meshnoise
    from .dataset import read_original
    dev = _device(opt.gpu)
    try:
        options = meshnoise.NoiseOptions(opt.levels, opt.kind, opt.direction, opt.fraction, opt.seed)
    except ValueError as e:
        print('noise: %s' % e, file=sys.stderr)
        return 1
    originals = folders.obj_files(os.path.join(opt.data_dir, 'original'))
    out_dir = opt.out_dir or os.path.join(opt.data_dir, 'noisy')
    os.makedirs(out_dir, exist_ok=True)
    print('\nNoise %s / %s, levels %s, seed %d, %d files ...\n'
          % (options.kind, options.direction, ','.join('%g' % v for v in options.levels), options.seed, len(originals)),
          flush=True)

    def one(original, skip):
        name = folders.stem_of(original)
        points, faces = read_original(original)
        geom = meshnoise.MeshGeometry(points, faces, dev)
        for k, level in enumerate(options.levels, 1):
            noisy = geom.draw(level, options.kind, options.direction, options.fraction, options.seed,
                              meshnoise.stream_of(name), k)
            out_file = os.path.join(out_dir, meshnoise.noisy_name(name, k) + '.obj')
            meshio.write_obj(out_file, noisy.cpu().numpy(), faces)
            print("V: %7d,  F: %7d,  L: %.6g,  sigma: %.6g,  '%s'"
                  % (points.shape[0], faces.shape[0], geom.mean_edge, geom.sigma(level), os.path.basename(out_file)),
                  flush=True)

    return folders.walk(originals, one)


def sample(opt):
    """Every DIR/original/*.obj, or else DIR/*.obj -> OUT/NAME.obj: --n points drawn by area on its surface (meshsample),
    `v` lines only, with --normals a `vn` line per point (the normal of the point's face)."""
    from . import meshin, meshio, meshnoise, meshsample
    dev = _device(opt.gpu)
    files = folders.originals(opt.data_dir)[0]
    out_dir = opt.out_dir or os.path.join(opt.data_dir, 'samples')
    os.makedirs(out_dir, exist_ok=True)
    print('\nSample, n %d, seed %d, normals %s, %d files ...\n' % (opt.n, opt.seed, 'on' if opt.normals else 'off', len(files)),
          flush=True)

    def one(path, skip):
        points, faces = meshio.read_obj(path)
        if faces.shape[0] == 0:
            raise ValueError('%s: no faces' % path)
        p, fv = meshin.device_mesh(points, faces, dev)
        weights = meshsample.surface_weights(p, fv, check=False)
        area, zero = meshsample.surface_info(weights)
        drawn = meshsample.sample_surface(p, fv, opt.n, seed=opt.seed, stream_id=meshnoise.stream_of(folders.stem_of(path)),
                                          weights=weights, check=False)
        normals = meshsample.sample_normals(p, fv, drawn).cpu().numpy() if opt.normals else None
        out_file = os.path.join(out_dir, os.path.basename(path))
        meshio.write_obj(out_file, drawn.points.cpu().numpy(), np.zeros((0, 3), dtype=np.int32), normals=normals)
        print("V: %7d,  F: %7d,  area: %.6g,  zero_faces: %d,  samples: %d,  '%s'"
              % (points.shape[0], faces.shape[0], area, zero, opt.n, os.path.basename(out_file)), flush=True)

    return folders.walk(files, one)


def _weld_tol(opt):
    return None if opt.no_weld else opt.weld_tol


def _topo_args(opt):
    """--orient / --min_component / --drop_intersecting as clean_mesh takes them (none is in the options without its flag)"""
    args = {'orient': getattr(opt, 'orient', False), 'min_component': getattr(opt, 'min_component', 0),
            'drop_intersecting': getattr(opt, 'drop_intersecting', False)}
    if getattr(opt, 'outward', False):         # --outward (meshwind.py): the key exists only with the flag
        args['outward'] = True
    return args


def _host_mesh(result):
    """what a mesh tool made, as the arrays write_obj takes"""
    return result.points.cpu().numpy(), result.faces.cpu().numpy()


def _clean_line(cleaned, V, F, out_file):
    c, t = cleaned.counts, cleaned.topology
    line = ("V: %7d -> %7d,  F: %7d -> %7d,  welded: %d,  degenerate: %d,  nonmanifold: %d,  unreferenced: %d,  rounds: %d,  '%s'"
            % (V, cleaned.points.shape[0], F, cleaned.faces.shape[0], c['welded'], c['degenerate'], c['nonmanifold'],
               c['unreferenced'], c['rounds'], os.path.basename(out_file)))
    if t is not None:          # '-': the stage that counts it was not asked for
        line += ',  ' + ',  '.join('%s: %s' % (label, t.get(key, '-')) for label, key in (
            ('flipped', 'flipped'), ('nonorientable', 'nonorientable'), ('components', 'components'), ('small', 'faces_dropped')))
    if 'intersecting' in c:    # only with --drop_intersecting
        line += ',  intersecting: %d' % c['intersecting']
    if t is not None and 'turned' in t:        # only with --outward
        line += ',  turned: %d,  open_components: %d' % (t['turned'], t['open_components'])
    return line


def clean(opt):
    """Repair every mesh of a folder on the device (meshclean): with DIR/original, original/NAME.obj -> OUT/original/NAME.obj
    and the same maps on every noisy/NAME_n*.obj of the same size -> OUT/noisy/; else DIR/*.obj -> OUT/NAME.obj."""
    from . import meshclean
    dev = _device(opt.gpu)
    weld_tol = _weld_tol(opt)

    def plan(points, faces, path):
        cleaned = meshclean.clean_mesh(points, faces, weld_tol=weld_tol, manifold=not opt.no_manifold, device=dev,
                                       **_topo_args(opt))
        if cleaned.faces.shape[0] == 0:
            raise ValueError('%s: no faces left after cleaning' % path)
        return cleaned

    title = 'Clean, weld %s, half-edge rule %s' % (
        'off' if weld_tol is None else ('exact' if weld_tol == 0 else 'grid %g' % weld_tol), 'off' if opt.no_manifold else 'on')
    # the maps index a numpy array as it is: a paired array never goes to the device
    return folders.paired_walk(opt.data_dir, opt.out_dir or os.path.join(opt.data_dir, 'clean'), title, plan, _host_mesh,
                               _clean_line, meshclean.apply)


def _subdivide_line(refined, V, F, out_file):
    c = refined.counts
    return ("V: %7d -> %7d,  F: %7d -> %7d,  edges: %d,  split: %d,  boundary: %d,  complex: %d,  passes: %d,  '%s'"
            % (V, refined.points.shape[0], F, refined.faces.shape[0], c['edges'], c['split'], c['boundary_edges'],
               c['complex_edges'], c['passes'], os.path.basename(out_file)))


def subdivide(opt):
    """Refine every mesh of a folder on the device (meshsubdiv), with the folders of `clean`: with DIR/original,
    original/NAME.obj -> OUT/original/NAME.obj and the same plan on every noisy/NAME_n*.obj of the same size -> OUT/noisy/;
    else DIR/*.obj -> OUT/NAME.obj."""
    from . import meshin, meshsubdiv
    dev = _device(opt.gpu)

    def plan(points, faces, path):
        max_edge = opt.max_edge
        if opt.max_edge_diag is not None:
            max_edge = opt.max_edge_diag * meshin.bbox_diagonal(points)
        return meshsubdiv.subdivide(points, faces, levels=opt.levels, scheme=opt.scheme, max_edge=max_edge,
                                    max_rounds=opt.max_rounds, device=dev)

    mode = ('max_edge %g' % opt.max_edge if opt.max_edge is not None else
            'max_edge %g of the diagonal' % opt.max_edge_diag if opt.max_edge_diag is not None else
            '%s, levels %d' % (opt.scheme, opt.levels))
    return folders.paired_walk(opt.data_dir, opt.out_dir or os.path.join(opt.data_dir, 'subdivided'), 'Subdivide, ' + mode,
                               plan, _host_mesh, _subdivide_line, lambda r, p: meshsubdiv.apply(r, p).cpu().numpy())


def _fill_line(filled, V, F, out_file):
    c = filled.counts
    line = ("V: %7d -> %7d,  F: %7d -> %7d,  boundary: %d,  loops: %d,  filled: %d,  skipped: %d,  blocked: %d,  chain: %d,  '%s'"
            % (V, filled.points.shape[0], F, filled.faces.shape[0], c['boundary_edges'], c['loops'],
               c['filled_loops'], c['skipped_loops'], c['blocked_vertices'], c['chain_edges'], os.path.basename(out_file)))
    return line + (',  run clean --orient first' if c['blocked_vertices'] or c['chain_edges'] else '')


def fill(opt):
    """Close the holes of every mesh of a folder on the device (meshfill), with the folders of `subdivide`: with
    DIR/original, original/NAME.obj -> OUT/original/NAME.obj and the same fill on every noisy/NAME_n*.obj of the same size
    -> OUT/noisy/; else DIR/*.obj -> OUT/NAME.obj."""
    from . import meshfill
    dev = _device(opt.gpu)

    def plan(points, faces, path):
        return meshfill.fill_holes(points, faces, max_hole_edges=opt.max_hole_edges, device=dev)

    title = 'Fill, %s' % ('loops of at most %d edges' % opt.max_hole_edges if opt.max_hole_edges else 'every loop')
    return folders.paired_walk(opt.data_dir, opt.out_dir or os.path.join(opt.data_dir, 'filled'), title,
                               plan, _host_mesh, _fill_line, lambda r, p: meshfill.apply(r, p).cpu().numpy())


INFO_KEYS = ('vertices_used', 'faces', 'degenerate', 'edges', 'boundary_edges', 'complex_edges', 'inconsistent_edges',
             'components', 'orient_components', 'nonorientable', 'would_flip', 'euler')
INTERSECTION_KEYS = ('intersecting_pairs', 'intersecting_faces', 'folded_pairs')      # info --intersections
SOLID_KEYS = ('closed_components', 'inward_components')                                # info --solid, behind volume


def info(opt):
    """One meshtopo.mesh_report line per DIR/original/*.obj if that folder exists, else per DIR/*.obj."""
    from . import meshio, meshtopo
    dev = _device(opt.gpu)
    files = folders.originals(opt.data_dir)[0]
    weld_tol = _weld_tol(opt)
    print('\nInfo, weld %s, %d files ...\n'
          % ('off' if weld_tol is None else ('exact' if weld_tol == 0 else 'grid %g' % weld_tol), len(files)), flush=True)

    def one(path, skip):
        points, faces = meshio.read_obj(path)
        more = {'solid': True} if opt.solid else {}
        r = meshtopo.mesh_report(points, faces, weld_tol=weld_tol, device=dev, intersections=opt.intersections, **more)
        line = ("V: %7d,  F: %7d,  %s,  closed: %s,  '%s'"
                % (points.shape[0], faces.shape[0], ',  '.join('%s: %d' % (k, r[k]) for k in INFO_KEYS),
                   'yes' if r['closed'] else 'no', os.path.basename(path)))
        if opt.intersections:
            line += ',  ' + ',  '.join('%s: %d' % (k, r[k]) for k in INTERSECTION_KEYS)
        if opt.solid:
            line += ',  volume: %.9g,  ' % r['volume'] + ',  '.join('%s: %d' % (k, r[k]) for k in SOLID_KEYS)
        print(line, flush=True)

    return folders.walk(files, one)


def train(opt):
    from . import trainer
    trainer.require_single_process()              # before the device is touched
    trainer.require_known_losses(opt)
    return trainer.train(opt, _device(opt.gpu), predict=denoise)


def _decimate_line(decimated, V, F, out_file):
    c = decimated.counts
    return ("V: %7d -> %7d,  F: %7d -> %7d,  rounds: %d,  reached: %s,  '%s'"
            % (V, decimated.points.shape[0], F, decimated.faces.shape[0], c['rounds'], 'yes' if c['reached'] else 'no',
               os.path.basename(out_file)))


def decimate(opt):
    """Simplify every mesh of a folder on the device (meshdecim), with the folders of `subdivide`: with DIR/original,
    original/NAME.obj -> OUT/original/NAME.obj and the same collapses on every noisy/NAME_n*.obj of the same size ->
    OUT/noisy/; else DIR/*.obj -> OUT/NAME.obj."""
    from . import meshdecim
    dev = _device(opt.gpu)

    def plan(points, faces, path):
        return meshdecim.decimate(points, faces, target_faces=opt.faces, ratio=opt.ratio, max_cost=opt.max_cost,
                                  max_rounds=opt.max_rounds, device=dev)

    mode = ('to %d faces' % opt.faces if opt.faces is not None else 'to %g of the faces' % opt.ratio)
    if opt.max_cost is not None:
        mode += ', max_cost %g' % opt.max_cost
    return folders.paired_walk(opt.data_dir, opt.out_dir or os.path.join(opt.data_dir, 'decimated'), 'Decimate, ' + mode,
                               plan, _host_mesh, _decimate_line, lambda r, p: meshdecim.apply(r, p).cpu().numpy())


def _remesh_line(r, V, F, drift, out_file):
    return ("V: %7d -> %7d,  F: %7d -> %7d,  in [low, high]: %5.1f%% -> %5.1f%%,  valence dev: %.3f -> %.3f,  "
            "drift mean: %.3e,  max: %.3e,  '%s'"
            % (V, r.points.shape[0], F, r.faces.shape[0], 100.0 * r.before['share'], 100.0 * r.after['share'],
               r.before['valence_dev'], r.after['valence_dev'], drift[0], drift[1], os.path.basename(out_file)))


def remesh(opt):
    """Remesh every mesh of a folder on the device (meshremesh), with the folders of `decimate`: DIR/original/NAME.obj ->
    OUT/original/NAME.obj if DIR/original exists, else DIR/*.obj -> OUT/NAME.obj.  Relaxation is no replayable map, so the
    files of DIR/noisy are NOT carried along -- unless --project is given: then every iteration ends on the input surface,
    every output vertex has an address on it, and with DIR/noisy present every noisy/NAME_n*.obj of equal size is written to
    OUT/noisy through that map (the paired walk of `decimate`)."""
    import torch
    from . import mesheval, meshin, meshio, meshremesh
    dev = _device(opt.gpu)
    out_dir = opt.out_dir or os.path.join(opt.data_dir, 'remeshed')
    mode = ('target edge %g' % opt.target_edge if opt.target_edge is not None else
            'target edge %g of the diagonal' % opt.target_edge_diag if opt.target_edge_diag is not None else
            'target edge = the mean edge')

    def run(points, faces):
        """-> (Remeshed, (mean, max) of the drift)"""
        r = meshremesh.remesh(points, faces, target_edge=opt.target_edge, target_edge_diag=opt.target_edge_diag,
                              iterations=opt.iterations, feature_angle=opt.feature_angle, relax_lambda=opt.relax_lambda,
                              max_rounds=opt.max_rounds, device=dev, project=opt.project, index=_index_of(opt))
        drift = (0.0, 0.0)
        if r.points.shape[0] and faces.shape[0]:         # the new vertices against the INPUT surface
            with torch.cuda.device(dev):
                d = mesheval.point_to_mesh(r.points, *meshin.device_mesh(points, faces, dev))[0]
            drift = (float(d.double().mean()), float(d.max()))
        return r, drift

    if opt.project and os.path.isdir(os.path.join(opt.data_dir, 'original')) and os.path.isdir(os.path.join(opt.data_dir, 'noisy')):
        return folders.paired_walk(opt.data_dir, out_dir, 'Remesh, %s, %d iterations, projected' % (mode, opt.iterations),
                                   lambda points, faces, path: run(points, faces), lambda rd: _host_mesh(rd[0]),
                                   lambda rd, V, F, out_file: _remesh_line(rd[0], V, F, rd[1], out_file),
                                   lambda rd, p: meshremesh.apply(rd[0], p).cpu().numpy())
    files, paired = folders.originals(opt.data_dir)
    out_original = os.path.join(out_dir, 'original') if paired else out_dir
    os.makedirs(out_original, exist_ok=True)
    print('\nRemesh, %s, %d iterations%s, %d files ...\n' % (mode, opt.iterations, ', projected' if opt.project else '',
                                                            len(files)), flush=True)
    if paired and not opt.project and os.path.isdir(os.path.join(opt.data_dir, 'noisy')):
        print('noisy/ is not carried along: the relaxed vertices have no counterpart in a paired file.  Make new pairs '
              'with `noise` on the output folder.\n', flush=True)

    def one(path, skip):
        points, faces = meshio.read_obj(path)
        r, drift = run(points, faces)
        out_file = os.path.join(out_original, os.path.basename(path))
        meshio.write_obj(out_file, *_host_mesh(r))
        print(_remesh_line(r, points.shape[0], faces.shape[0], drift, out_file), flush=True)

    return folders.walk(files, one, of_total=False)


def project(opt):
    """The vertices of every source mesh of --data_dir moved to their closest points on the surface of its target of
    --target_dir (meshproject.project; the pairing of `align`), written to --out_dir with its own faces."""
    from . import meshin, meshio, meshproject
    dev = _device(opt.gpu)
    jobs = align_list(opt.data_dir, opt.target_dir)
    out_dir = opt.out_dir or os.path.join(opt.data_dir, 'projected')
    os.makedirs(out_dir, exist_ok=True)
    mode = ('max_dist %g' % opt.max_dist if opt.max_dist is not None else
            'max_dist %g of the diagonal' % opt.max_dist_diag if opt.max_dist_diag is not None else 'no max_dist')
    print('\nProject, %s, %d files ...\n' % (mode, len(jobs)), flush=True)

    def one(job, skip):
        source, target = job
        points, faces = meshio.read_obj(source)
        t_points, t_faces = meshio.read_obj(target)
        if points.shape[0] == 0:
            raise ValueError('%s has no vertices' % source)
        max_dist = opt.max_dist_diag * meshin.bbox_diagonal(t_points) if opt.max_dist_diag is not None else opt.max_dist
        out, kept, c = meshproject.project(points, t_points, t_faces, max_dist=max_dist, device=dev, index=_index_of(opt))
        out_file = os.path.join(out_dir, os.path.basename(source))
        meshio.write_obj(out_file, out.cpu().numpy(), faces)
        moved = (out - c.points.new_tensor(points)).double().norm(dim=1)
        print("V: %7d,  kept: %7d,  moved mean: %.6e,  max: %.6e,  '%s'"
              % (points.shape[0], kept, float(moved.mean()), float(moved.max()), os.path.basename(out_file)), flush=True)

    return folders.walk(jobs, one)


def _weld_tol_arg(text):
    v = float(text)
    if not (v >= 0.0 and v < float('inf')):
        raise argparse.ArgumentTypeError('--weld_tol is 0 (equal coordinates) or a positive cell size, not %r' % text)
    return v


def _min_component_arg(text):
    v = int(text)
    if v < 0:
        raise argparse.ArgumentTypeError('--min_component is 0 (keep every part) or a number of faces, not %r' % text)
    return v


def _samples_arg(text):
    from .meshin import MAX_NODES
    v = int(text)
    if not 0 <= v <= MAX_NODES:
        raise argparse.ArgumentTypeError('a number of samples is between 0 and 16 777 215, not %r' % text)
    return v


def _positive_arg(text):
    v = float(text)
    if not (v > 0.0 and v < float('inf')):
        raise argparse.ArgumentTypeError('a positive length, not %r' % text)
    return v


def _ratio_arg(text):
    v = float(text)
    if not 0.0 < v < 1.0:
        raise argparse.ArgumentTypeError('a part of the faces above 0 and below 1, not %r' % text)
    return v


def _not_negative_arg(text):
    v = float(text)
    if not (v >= 0.0 and v < float('inf')):
        raise argparse.ArgumentTypeError('0 or a positive number, not %r' % text)
    return v


def _count_arg(text):
    v = int(text)
    if v < 0:
        raise argparse.ArgumentTypeError('a whole number, not negative, not %r' % text)
    return v


def _feature_angle_arg(text):
    v = float(text)
    if not (0.0 <= v <= 90.0 or v == 180.0):
        raise argparse.ArgumentTypeError('degrees in [0, 90], or 180 for no feature edges, not %r' % text)
    return v


def _unit_arg(text):
    v = float(text)
    if not 0.0 <= v <= 1.0:
        raise argparse.ArgumentTypeError('a number in [0, 1], not %r' % text)
    return v


def _at_least_one_arg(text):
    v = int(text)
    if v < 1:
        raise argparse.ArgumentTypeError('a whole number, at least 1, not %r' % text)
    return v


class _TrueGiven(argparse.Action):
    """store_true, and note in <dest>_given that the flag was on the command line"""

    def __init__(self, option_strings, dest, default=False, **kw):
        super().__init__(option_strings, dest, nargs=0, default=default, **kw)

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, True)
        setattr(namespace, self.dest + '_given', True)


def _add_clean_flags(p, given=False):
    p.add_argument('--weld_tol', type=_weld_tol_arg, default=0.0, action=_StoreGiven if given else 'store',
                   help='0: weld vertices with equal coordinates (default); > 0: weld the vertices of one grid cell of this '
                        'side (a snap to a grid, not an epsilon-merge)')
    p.add_argument('--no_weld', action=_TrueGiven, help='keep every vertex apart')
    p.add_argument('--no_manifold', action=_TrueGiven, help='keep faces that give a directed edge a second owner')
    # the two topology flags leave no entry in the options unless they are given: what `denoise` hands on stays as it was
    p.add_argument('--orient', action=_TrueGiven, default=argparse.SUPPRESS,
                   help='wind the faces of every connected part consistently (its lowest face decides) before the half-edge '
                        'rule')
    p.add_argument('--min_component', type=_min_component_arg, default=argparse.SUPPRESS, action=_StoreGiven, metavar='N',
                   help='drop the edge-connected parts of fewer than N faces')
    p.add_argument('--drop_intersecting', action=_TrueGiven, default=argparse.SUPPRESS,
                   help='drop the faces that intersect another face (all pairs, on the welded table); `fill` closes the '
                        'holes this opens')
    p.add_argument('--outward', action=_TrueGiven, default=argparse.SUPPRESS,
                   help='--orient, and then every closed part is wound so that its normals point out of the solid: a part of '
                        'negative volume is turned, and a part nested at odd depth in the others (a cavity) is turned back')


def build_parser():
    ap = argparse.ArgumentParser(prog='python -m geobi_gnn_amd', description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='command', required=True)
    d = sub.add_parser('denoise', help='denoise every OBJ mesh of a folder and write NAME-<n_iter>.obj')
    d.add_argument('--method', type=str, default='gnn', choices=['gnn', 'bnf', 'gnf'],
                   help='gnn: the network (default); bnf: bilateral normal filter; gnf: guided normal filter; the filters '
                        'need no model')
    d.add_argument('--model', type=str, default='', help="state dict with the reference's keys; random init (seed 0) if empty")
    d.add_argument('--data_dir', type=str, required=True)
    d.add_argument('--out_dir', type=str, default='', help='default: <data_dir>/result')
    d.add_argument('--sub_size', type=int, default=20000, help='faces per patch')
    d.add_argument('--n_iter', type=int, default=60, action=_StoreGiven,
                   help='vertex-update sweeps (--method bnf / gnf: 20 unless given)')
    d.add_argument('--normal_iters', type=int, default=20, help='bnf, gnf: sweeps of the normal filter')
    d.add_argument('--sigma_r', type=float, default=0.35, help='bnf, gnf: range width, on |n_i - n_j| (gnf: of the guidance normals)')
    d.add_argument('--sigma_s', type=float, default=1.0, help='bnf, gnf: spatial width in units of the mean centroid distance')
    d.add_argument('--data_type', type=str, default='Synthetic', choices=['Synthetic', 'Kinect_v1', 'Kinect_v2', 'Kinect_Fusion'])
    d.add_argument('--wei_param', type=int, default=2)
    d.add_argument('--force_depth', action='store_true')
    d.add_argument('--pool_type', type=str, default='max', choices=['max', 'mean'])
    d.add_argument('--gpu', type=int, default=-1, help='device index (default: the current device)')
    d.add_argument('--clean', action='store_true',
                   help='repair every file first (meshclean: weld, degenerate and non-manifold faces, unused vertices); the '
                        "result keeps the file's numbering and faces")
    _add_clean_flags(d, given=True)
    d.set_defaults(fn=denoise)
    e = sub.add_parser('eval', help='score result meshes against their originals, write ErrorInfo_h.txt')
    e.add_argument('--result_dir', type=str, required=True)
    e.add_argument('--original_dir', type=str, required=True)
    e.add_argument('--gpu', type=int, default=-1)
    e.add_argument('--align', action='store_true',
                   help='bring every result into the frame of its ground truth by rigid ICP first; writes AlignInfo.txt')
    e.add_argument('--scale', action='store_true', help='with --align: estimate a scale as well')
    e.add_argument('--free', action='store_true',
                   help='score pairs whose vertex counts or face tables differ (surface distances both ways, normals by the '
                        'nearest ground-truth triangle); writes ErrorInfo_free.txt')
    e.add_argument('--samples', type=_samples_arg, default=0, metavar='N',
                   help='with --free: also score from N points drawn by area on each surface; writes ErrorInfo_sampled.txt '
                        '(with --align the ground truth is aligned to as its vertices plus its samples)')
    e.add_argument('--signed', action='store_true',
                   help="with --free: also the mean SIGNED distance of the result's vertices to the ground truth (negative "
                        'inside), the share of vertices inside and the volume ratio; writes ErrorInfo_signed.txt')
    e.add_argument('--seed', type=int, default=1, help='with --samples: the seed of the draw')
    e.add_argument('--index', type=str, choices=('none', 'grid'), default='none',
                   help='none: the searches walk all pairs; grid: a uniform grid in front of them, the same bits (DESIGN.md 4u)')
    e.set_defaults(fn=evaluate)
    a = sub.add_parser('align', help='align every mesh of a folder to its target by rigid ICP and write it with its own faces')
    a.add_argument('--data_dir', type=str, required=True, help='the meshes to move: NAME_*.obj, or NAME.obj')
    a.add_argument('--target_dir', type=str, required=True, help='holds the targets NAME.obj')
    a.add_argument('--out_dir', type=str, default='', help='default: <data_dir>/aligned')
    a.add_argument('--scale', action='store_true', help='estimate a scale as well (a similarity instead of a rigid motion)')
    a.add_argument('--reflect', action='store_true', help='allow reflections (det R = -1)')
    a.add_argument('--max_iter', type=int, default=100, help='iterations at most; a pair that hits it is written and reported')
    a.add_argument('--rmse_thr', type=float, default=1e-6, help='stop once the relative change of the rmse is at most this')
    a.add_argument('--samples', type=_samples_arg, default=0, metavar='N',
                   help="align to the target's vertices followed by N points drawn by area on its surface (a CAD target of "
                        'a few large triangles has no vertices inside its faces)')
    a.add_argument('--seed', type=int, default=1, help='with --samples: the seed of the draw')
    a.add_argument('--gpu', type=int, default=-1)
    a.set_defaults(fn=align)
    s = sub.add_parser('sample', help='write N points drawn uniformly by area on the surface of every mesh of a folder')
    s.add_argument('--data_dir', type=str, required=True, help='holds original/, or the OBJ files themselves')
    s.add_argument('--out_dir', type=str, default='', help='default: <data_dir>/samples')
    s.add_argument('--n', type=_samples_arg, required=True, help='points per mesh')
    s.add_argument('--seed', type=int, default=1)
    s.add_argument('--normals', action='store_true', help="a `vn` line per point: the unit normal of the point's face")
    s.add_argument('--gpu', type=int, default=-1)
    s.set_defaults(fn=sample)
    n = sub.add_parser('noise', help='write noisy/NAME_n<k>.obj for every original/NAME.obj, drawn on the device')
    from .meshnoise import DIRECTIONS, KINDS
    from .trainer import noise_levels_arg
    n.add_argument('--data_dir', type=str, required=True, help='holds original/')
    n.add_argument('--levels', type=noise_levels_arg, default=[0.1, 0.2, 0.3],
                   help='noise levels as fractions of the mean edge length; level k of the list goes to NAME_n<k>.obj')
    n.add_argument('--kind', type=str, default='gaussian', choices=list(KINDS))
    n.add_argument('--direction', type=str, default='normal', choices=list(DIRECTIONS))
    n.add_argument('--fraction', type=float, default=0.3, help='share of the vertices the impulsive kind moves')
    n.add_argument('--seed', type=int, default=1)
    n.add_argument('--out_dir', type=str, default='', help='default: <data_dir>/noisy')
    n.add_argument('--gpu', type=int, default=-1)
    n.set_defaults(fn=noise)
    c = sub.add_parser('clean', help='weld vertices, drop degenerate / non-manifold faces and unused vertices, on the device')
    c.add_argument('--data_dir', type=str, required=True, help='holds original/ (and noisy/), or the OBJ files themselves')
    c.add_argument('--out_dir', type=str, default='', help='default: <data_dir>/clean')
    _add_clean_flags(c)
    c.add_argument('--gpu', type=int, default=-1)
    c.set_defaults(fn=clean)
    i = sub.add_parser('info', help='edges, boundary / complex / inconsistent edges, parts, closed, orientable: one line per mesh')
    i.add_argument('--data_dir', type=str, required=True, help='holds original/, or the OBJ files themselves')
    i.add_argument('--weld_tol', type=_weld_tol_arg, default=0.0, help='as for clean: the report is computed after the weld')
    i.add_argument('--no_weld', action='store_true', help='keep every vertex apart')
    i.add_argument('--intersections', action='store_true',
                   help='also count the pairs of faces that intersect, the faces in such a pair and the pairs folded flat onto '
                        'each other (all pairs of faces: F * F box tests)')
    i.add_argument('--solid', action='store_true',
                   help='also the volume the closed parts enclose as the file winds them, their number, and how many of them '
                        '`clean --outward` would turn (all pairs of parts and faces)')
    i.add_argument('--gpu', type=int, default=-1)
    i.set_defaults(fn=info)
    u = sub.add_parser('subdivide', help='make every mesh denser on the device: midpoint or Loop passes, or split the edges '
                                         'longer than a length')
    u.add_argument('--data_dir', type=str, required=True, help='holds original/ (and noisy/), or the OBJ files themselves')
    u.add_argument('--out_dir', type=str, default='', help='default: <data_dir>/subdivided')
    u.add_argument('--levels', type=_at_least_one_arg, default=1, action=_StoreGiven,
                   help='uniform passes; each splits every edge and makes four faces of one')
    u.add_argument('--scheme', type=str, default='midpoint', choices=['midpoint', 'loop'],
                   help='midpoint: the surface stays as it is (default); loop: smoothed positions, edges that are not shared '
                        'by exactly two faces are creases')
    u.add_argument('--max_edge', type=_positive_arg, default=None, metavar='L',
                   help='split only the edges longer than L, in rounds, until none is left')
    u.add_argument('--max_edge_diag', type=_positive_arg, default=None, metavar='R',
                   help="--max_edge as R times the diagonal of the mesh's bounding box")
    u.add_argument('--max_rounds', type=_at_least_one_arg, default=16, help='with --max_edge*: rounds at most')
    u.add_argument('--gpu', type=int, default=-1)
    u.set_defaults(fn=subdivide)
    k = sub.add_parser('decimate', help='make every mesh coarser on the device: rounds of quadric edge collapses down to a '
                                        'face count, boundaries kept')
    k.add_argument('--data_dir', type=str, required=True, help='holds original/ (and noisy/), or the OBJ files themselves')
    k.add_argument('--out_dir', type=str, default='', help='default: <data_dir>/decimated')
    stop = k.add_mutually_exclusive_group(required=True)
    stop.add_argument('--ratio', type=_ratio_arg, default=None, metavar='R', help='stop at R times the faces of each mesh')
    stop.add_argument('--faces', type=_count_arg, default=None, metavar='N', help='stop at N faces (or one below)')
    k.add_argument('--max_cost', type=_not_negative_arg, default=None, metavar='C',
                   help='collapse no edge whose quadric cost is above C (0: only what leaves the surface as it is)')
    k.add_argument('--max_rounds', type=_at_least_one_arg, default=256, help='rounds at most')
    k.add_argument('--gpu', type=int, default=-1)
    k.set_defaults(fn=decimate)
    r = sub.add_parser('remesh', help='make every mesh regular on the device: split long edges, collapse short ones, flip '
                                      'towards valence 6, relax tangentially')
    r.add_argument('--data_dir', type=str, required=True, help='holds original/, or the OBJ files themselves')
    r.add_argument('--out_dir', type=str, default='', help='default: <data_dir>/remeshed')
    edge = r.add_mutually_exclusive_group()
    edge.add_argument('--target_edge', type=_positive_arg, default=None, metavar='L',
                      help='the edge length to aim at (default: the mean edge length of each mesh)')
    edge.add_argument('--target_edge_diag', type=_positive_arg, default=None, metavar='R',
                      help="--target_edge as R times the diagonal of the mesh's bounding box")
    r.add_argument('--iterations', type=_count_arg, default=5, help='split / collapse / flip / relax iterations')
    r.add_argument('--feature_angle', type=_feature_angle_arg, default=40.0, metavar='DEG',
                   help='edges whose faces meet at more than DEG degrees (0 .. 90) keep their vertices; 180: none')
    r.add_argument('--relax_lambda', type=_unit_arg, default=0.5, help='the step of the relaxation, in [0, 1]')
    r.add_argument('--max_rounds', type=_at_least_one_arg, default=64, help='rounds at most in each inner loop')
    r.add_argument('--project', action='store_true',
                   help='end every iteration by moving the relaxed vertices to their closest points on the input surface; '
                        'with <data_dir>/noisy present its files are carried along to <out_dir>/noisy')
    r.add_argument('--index', type=str, choices=('none', 'grid'), default='none',
                   help='none: the searches walk all pairs; grid: a uniform grid in front of them, the same bits (DESIGN.md 4u)')
    r.add_argument('--gpu', type=int, default=-1)
    r.set_defaults(fn=remesh)
    j = sub.add_parser('project', help='move the vertices of every mesh of a folder to their closest points on the surface '
                                       'of its target and write it with its own faces')
    j.add_argument('--data_dir', type=str, required=True, help='the meshes to move: NAME_*.obj, or NAME.obj')
    j.add_argument('--target_dir', type=str, required=True, help='holds the targets NAME.obj')
    j.add_argument('--out_dir', type=str, default='', help='default: <data_dir>/projected')
    far = j.add_mutually_exclusive_group()
    far.add_argument('--max_dist', type=_not_negative_arg, default=None, metavar='D',
                     help='a vertex farther than D from the surface stays where it is')
    far.add_argument('--max_dist_diag', type=_not_negative_arg, default=None, metavar='R',
                     help="--max_dist as R times the diagonal of the target's bounding box")
    j.add_argument('--index', type=str, choices=('none', 'grid'), default='none',
                   help='none: the searches walk all pairs; grid: a uniform grid in front of them, the same bits (DESIGN.md 4u)')
    j.add_argument('--gpu', type=int, default=-1)
    j.set_defaults(fn=project)
    h = sub.add_parser('fill', help='close the holes of every mesh on the device: one new vertex and a fan of faces per '
                                    'closed boundary loop')
    h.add_argument('--data_dir', type=str, required=True, help='holds original/ (and noisy/), or the OBJ files themselves')
    h.add_argument('--out_dir', type=str, default='', help='default: <data_dir>/filled')
    h.add_argument('--max_hole_edges', type=_count_arg, default=0, metavar='N',
                   help='fill only the loops of at most N edges (0, the default: every loop)')
    h.add_argument('--gpu', type=int, default=-1)
    h.set_defaults(fn=fill)
    t = sub.add_parser('train', help='train on <data_dir>/train, evaluate on <data_dir>/test, keep the best model')
    from .trainer import add_train_flags
    add_train_flags(t)
    t.set_defaults(fn=train)
    return ap


def parse_args(argv=None):
    ap = build_parser()
    opt = ap.parse_args(argv)
    if opt.command == 'denoise':
        if opt.method in ('bnf', 'gnf') and opt.model:
            ap.error('denoise: --model cannot be combined with --method %s (the filter has no model)' % opt.method)
        if opt.method in ('bnf', 'gnf') and (opt.normal_iters < 0 or not opt.sigma_r > 0 or not opt.sigma_s > 0 or opt.n_iter < 0):
            ap.error('denoise: --normal_iters and --n_iter are not negative, --sigma_r and --sigma_s positive')
        if not opt.clean:
            for flag in ('weld_tol', 'no_weld', 'no_manifold', 'orient', 'min_component', 'drop_intersecting', 'outward'):
                if getattr(opt, flag + '_given', False):
                    ap.error('denoise: --%s needs --clean' % flag)
    if opt.command == 'remesh' and opt.index != 'none' and not opt.project:
        ap.error('remesh: --index serves the searches of --project')
    if opt.command == 'eval' and opt.scale and not opt.align:
        ap.error('eval: --scale needs --align')
    if opt.command == 'eval' and opt.samples and not opt.free:
        ap.error('eval: --samples needs --free')
    if opt.command == 'eval' and opt.signed and not opt.free:
        ap.error('eval: --signed needs --free')
    if opt.command in ('eval', 'align', 'sample') and not 0 <= opt.seed < 2 ** 64:
        ap.error('%s: --seed is a 64-bit number that is not negative, got %d' % (opt.command, opt.seed))
    if opt.command == 'align':
        if opt.max_iter < 1:
            ap.error('align: --max_iter is at least 1, not %d' % opt.max_iter)
        if not opt.rmse_thr >= 0:
            ap.error('align: --rmse_thr is not negative, got %r' % opt.rmse_thr)
    if opt.command == 'subdivide':
        if opt.max_edge is not None and opt.max_edge_diag is not None:
            ap.error('subdivide: --max_edge and --max_edge_diag exclude each other')
        if opt.max_edge is not None or opt.max_edge_diag is not None:
            if getattr(opt, 'levels_given', False):
                ap.error('subdivide: --max_edge / --max_edge_diag run rounds until no edge is longer; --levels does not apply')
            if opt.scheme == 'loop':
                ap.error('subdivide: --max_edge / --max_edge_diag split at midpoints; --scheme loop does not apply')
    return opt


def main(argv=None):
    opt = parse_args(argv)
    return opt.fn(opt)


if __name__ == '__main__':
    sys.exit(main())
