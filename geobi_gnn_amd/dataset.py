"""Training samples from folders of OBJ meshes, resident on the device: the counterpart of
code/dataset.py:72-276 of the reference (``DualDataset``).

Layout of the reference (``dataset/<data_type>``):

  <root>/<split>/original/NAME.obj          ground truth
  <root>/<split>/noisy/NAME_n*.obj          its noisy copies (same connectivity)
  <root>/<split>/processed_data/SAMPLE.pt   cache of the preprocessed samples (data.save_processed)
  <root>/<list>.txt                         optional list of NAMEs (train_list.txt / test_list.txt)

With ``noise=`` the split needs ``original/`` only: the noisy copies are drawn on the device (meshnoise: one Philox stream
per NAME, one draw per level and resampling round), nothing is cached, and ``resample(d)`` replaces every sample by its
draw-``d`` version -- bit-identical to a file-mode dataset over noise files written from the same draws.

A mesh of at most ``submesh_size`` faces is one sample; a larger one is cut into patches exactly as inference cuts it
(patches.split_faces: dataset.py:156-193), every patch normalised by the WHOLE noisy mesh's centroid and scale, and
patches of at most ``filter_patch_count`` faces are dropped.  Preprocessing runs on the device
(meshprep.build_dual_data); the samples stay there with everything that depends on one mesh built once, so a training
step's batch is data.union_batch_graphs over resident pairs -- which always copies: nothing downstream writes a sample.
"""
import os
import sys

import torch

from . import _lib as L
from . import folders, meshio, meshnoise, meshprep, patches
from .data import load_processed, save_processed

PROCESSED_FOLDER = 'processed_data'


def _originals(root, split, data_list_txt):
    """[(NAME, original file)]: the names of ``<root>/<data_list_txt>`` or of the sorted ``<split>/original/*.obj``; a
    listed name without an original file is reported on stderr and left out."""
    original_dir = os.path.join(root, split, 'original')
    if data_list_txt is not None:
        with open(os.path.join(root, data_list_txt)) as fh:
            names = [ln.strip() for ln in fh if ln.strip()]
    else:
        names = [folders.stem_of(f) for f in folders.obj_files(original_dir)]
    found = []
    for name in names:
        original = os.path.join(original_dir, name + '.obj')
        if not os.path.isfile(original):
            print('skipped: %s has no original file %s' % (name, original), file=sys.stderr, flush=True)
            continue
        found.append((name, original))
    return found


def original_files(root, split, data_list_txt=None):
    """[(NAME, original file)] of one split, host only: the names of ``file_pairs`` without the noisy side.  None at all
    is a ValueError."""
    found = _originals(root, split, data_list_txt)
    if not found:
        raise ValueError('no original mesh under %s' % os.path.join(root, split))
    return found


def file_pairs(root, split, data_list_txt=None):
    """[(noisy file, original file)] of one split (dataset.py:83-103), host only.  Names come from
    ``<root>/<data_list_txt>`` (blank lines dropped, list order kept) or from the sorted ``<split>/original/*.obj``;
    each pairs with its sorted ``<split>/noisy/<name>_n*.obj`` (the pattern of the ``denoise`` command).  A listed name
    without an original or without a noisy file is reported on stderr and skipped; no pair at all is a ValueError."""
    noisy_dir = os.path.join(root, split, 'noisy')
    pairs = []
    for name, original in _originals(root, split, data_list_txt):
        noisy = folders.noisy_of(noisy_dir, name)
        if not noisy:
            print('skipped: %s has no noisy file %s' % (name, os.path.join(noisy_dir, name + '_n*.obj')), file=sys.stderr,
                  flush=True)
            continue
        pairs += [(n, original) for n in noisy]
    if not pairs:
        raise ValueError('no (noisy, original) pairs under %s' % os.path.join(root, split))
    return pairs


def read_original(original_file):
    """-> (points, faces) of a clean mesh, with the per-file checks of the ``denoise`` command: at least one face, every
    vertex referenced by a face.  ValueError names the file."""
    points, faces = meshio.read_obj(original_file)
    if faces.shape[0] == 0:
        raise ValueError('%s: no faces' % original_file)
    loose = meshio.unreferenced_vertices(points.shape[0], faces)
    if loose:
        raise ValueError('%s: %d of %d vertices are referenced by no face' % (original_file, loose, points.shape[0]))
    return points, faces


def read_pair(noisy_file, original_file):
    """-> (noisy points, faces, original points), with the checks of the ``denoise`` command: at least one face, every
    vertex referenced by a face, both files of one size.  ValueError names the file."""
    points, faces = meshio.read_obj(noisy_file)
    if faces.shape[0] == 0:
        raise ValueError('%s: no faces' % noisy_file)
    loose = meshio.unreferenced_vertices(points.shape[0], faces)
    if loose:
        raise ValueError('%s: %d of %d vertices are referenced by no face' % (noisy_file, loose, points.shape[0]))
    gt_points, gt_faces = meshio.read_obj(original_file)
    if gt_points.shape != points.shape or gt_faces.shape != faces.shape:
        raise ValueError('%s (V = %d, F = %d) and its ground truth %s (V = %d, F = %d) differ in size'
                         % (noisy_file, points.shape[0], faces.shape[0], original_file, gt_points.shape[0],
                            gt_faces.shape[0]))
    return points, faces, gt_points


class DualDataset(object):
    """``dataset[i]`` -> the resident (data_v, data_f) of sample ``i``; ``names[i]`` its name (the noisy file's stem, or
    ``<stem>-sub<submesh_size>-<seed face id>`` for a patch).  cache=False neither reads nor writes ``processed_data``.
    noise: a meshnoise.NoiseOptions or a dict of its arguments (levels, kind, direction, fraction, seed): the samples of
    (NAME, level k) are named ``NAME_n<k>`` and drawn from ``original/NAME.obj`` on the device (never cached)."""

    def __init__(self, root, split='train', data_list_txt=None, submesh_size=20000, filter_patch_count=0,
                 data_type='Synthetic', device=None, cache=True, noise=None):
        if not torch.cuda.is_available():
            raise L.GeobiError('DualDataset preprocesses and keeps its samples on the MI355X (no CPU fallback)')
        self.root, self.split, self.data_type = root, split, data_type
        self.submesh_size, self.filter_patch_count = int(submesh_size), int(filter_patch_count)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.noise = meshnoise.NoiseOptions.of(noise)
        self.cache = bool(cache) and self.noise is None
        self.processed_dir = os.path.join(root, split, PROCESSED_FOLDER)
        self.names, self.samples, self.skipped = [], [], 0
        self.draw = 0
        if self.noise is not None:
            self._synthesise(original_files(root, split, data_list_txt))
        else:
            self.pairs = file_pairs(root, split, data_list_txt)
            if self.cache:
                os.makedirs(self.processed_dir, exist_ok=True)
            for noisy_file, original_file in self.pairs:
                try:
                    self._process_pair(noisy_file, original_file)
                except (ValueError, OSError, L.GeobiError) as e:
                    self.skipped += 1
                    print('skipped: %s' % e, file=sys.stderr, flush=True)
        if not self.samples:
            raise ValueError('no usable sample under %s' % os.path.join(root, split))

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        return self.samples[i]

    # ------------------------------------------------------------------ one (noisy, original) pair
    def _process_pair(self, noisy_file, original_file):
        """process_one_data (dataset.py:130-194)."""
        points, faces, gt_points = read_pair(noisy_file, original_file)
        self._process_arrays(os.path.basename(noisy_file)[:-4], points, faces, gt_points)

    def _process_arrays(self, stem, points, faces, gt_points, trusted_faces=False):
        """One (noisy, original) pair as host arrays (from files) or device tensors (drawn here; trusted_faces: the table
        was range-checked when the clean mesh was taken in)."""
        if faces.shape[0] <= self.submesh_size:
            self._add(stem, lambda: meshprep.build_dual_data(points, faces, points_gt=gt_points, name=stem,
                                                             data_type=self.data_type, device=self.device,
                                                             trusted_faces=trusted_faces))
            return
        dev = self.device
        pts = torch.as_tensor(points).to(dev)
        gt = torch.as_tensor(gt_points).to(dev)
        fv = torch.as_tensor(faces).to(dev).contiguous()           # read_obj checked the ids against V
        V = pts.shape[0]
        # centroid and scale of the whole noisy mesh, formed as patches.predict_mesh forms them
        rowptr, lst = meshprep.vertex_faces(fv, V)
        vf32 = meshprep.vf_padded32(rowptr, lst, V)
        g_v = meshprep.ring_graph(0, fv, rowptr, lst, V)
        centroid = pts.mean(0, keepdim=True)
        scale = float(1.0 / torch.tensor(meshprep.mean_edge_length(pts, g_v).tolist()[0], dtype=torch.float32))
        # the growth always runs (the next seed depends on every earlier patch, the names on the seeds); renumbering and
        # preprocessing only for a patch that is kept and not cached
        for sel in patches.split_faces(pts, fv, self.submesh_size, incidence=(rowptr, lst), vf32=vf32):
            if sel.shape[0] <= self.filter_patch_count:
                continue
            seed = L.read_i32(sel[:1], 1)[0]

            def build(sel=sel, name='%s-sub%d-%d' % (stem, self.submesh_size, seed)):
                v_idx, f_sub = patches.submesh(fv, sel, V)
                idx = v_idx.long()
                return meshprep.build_dual_data(pts[idx], f_sub, points_gt=gt[idx], name=name, data_type=self.data_type,
                                                device=dev, centroid=centroid, scale=scale, trusted_faces=True,
                                                want_vf=False)
            self._add('%s-sub%d-%d' % (stem, self.submesh_size, seed), build)

    def _add(self, name, build):
        path = os.path.join(self.processed_dir, name + '.pt')
        if self.cache and os.path.exists(path):
            data_v, data_f = load_processed(path, device=self.device)
        else:
            data_v, data_f = build()
            # meta holds the padded vertex -> face table and the incidence lists: they serve the vertex update of
            # inference only, and the cache format stores no tuples of device tensors
            data_v.meta = None
            if self.cache:
                save_processed((data_v, data_f), path)
        self.names.append(name)
        self.samples.append(_make_resident(data_v, data_f))

    # ------------------------------------------------------------------ noise drawn here
    def _synthesise(self, originals):
        """Take every clean mesh in once (points, face table, incidence, normals and mean edge length stay resident) and
        build the draw-0 samples of every (NAME, level)."""
        nz = self.noise
        self.pairs, self._entries = [], []
        for name, original_file in originals:
            self.pairs += [(meshnoise.noisy_name(name, k), original_file) for k in range(1, len(nz.levels) + 1)]
            try:
                points, faces = read_original(original_file)
                geom = meshnoise.MeshGeometry(points, faces, self.device)
            except (ValueError, OSError, L.GeobiError) as e:
                self.skipped += len(nz.levels)
                print('skipped: %s' % e, file=sys.stderr, flush=True)
                continue
            for k in range(1, len(nz.levels) + 1):
                self._entries.append({'name': name, 'k': k, 'geom': geom, 'faces': faces, 'first': 0, 'count': 0})
        self._rebuild(0, refresh=False)

    def noisy_points(self, entry, d=None):
        """Device points of one (NAME, level) entry at resampling round ``d`` (default: the current one)."""
        nz = self.noise
        return entry['geom'].draw(nz.levels[entry['k'] - 1], nz.kind, nz.direction, nz.fraction, nz.seed,
                                  meshnoise.stream_of(entry['name']), nz.draw_index(entry['k'], self.draw if d is None else d))

    def _rebuild(self, d, refresh):
        old_names, old_samples = self.names, self.samples
        self.names, self.samples, self.draw = [], [], int(d)
        for e in self._entries:
            geom, stem = e['geom'], meshnoise.noisy_name(e['name'], e['k'])
            first = len(self.samples)
            if refresh and e['count'] and geom.faces.shape[0] <= self.submesh_size:
                # same connectivity: the resident graphs, reverse-edge index and face table stay; only what moves is redone
                data_v, data_f = old_samples[e['first']]
                meshprep.refresh_dual_data(data_v, data_f, self.noisy_points(e), geom.points, self.data_type,
                                           incidence=geom.incidence)
                self.names.append(old_names[e['first']])
                self.samples.append((data_v, data_f))
            else:
                try:
                    self._process_arrays(stem, self.noisy_points(e), geom.faces, geom.points, trusted_faces=True)
                except (ValueError, L.GeobiError) as err:
                    if not refresh:
                        self.skipped += 1
                    print('skipped: %s: %s' % (stem, err), file=sys.stderr, flush=True)
            e['first'], e['count'] = first, len(self.samples) - first

    def resample(self, d):
        """Replace every sample by its draw-``d`` version (levels k = 1.. of round d use Philox draw k + len(levels) d).
        An unsplit mesh keeps its sample objects and graphs (meshprep.refresh_dual_data); a split one is cut again from
        the new noisy mesh, as a file-mode dataset over the new files would cut it."""
        if self.noise is None:
            raise ValueError('resample: this dataset reads its noisy meshes from files (no noise= options)')
        self._rebuild(d, refresh=True)
        if not self.samples:
            raise ValueError('no usable sample under %s after resample(%d)' % (os.path.join(self.root, self.split), d))

    def write_noisy(self, out_dir):
        """Write the current draw of every (NAME, level) as ``<out_dir>/NAME_n<k>.obj`` (meshio.write_obj) -> file list."""
        if self.noise is None:
            raise ValueError('write_noisy: this dataset reads its noisy meshes from files')
        os.makedirs(out_dir, exist_ok=True)
        files = []
        for e in self._entries:
            path = os.path.join(out_dir, meshnoise.noisy_name(e['name'], e['k']) + '.obj')
            meshio.write_obj(path, self.noisy_points(e).cpu().numpy(), e['faces'])
            files.append(path)
        return files


def _make_resident(data_v, data_f):
    """Everything that depends on ONE mesh, built once (what tools/train_synthetic.py does for its meshes): adjacency with
    the reverse-edge index, the validated int32 face table (a loaded table is range-checked here, once) and the
    vertex -> corner lists, so that data.union_batch_graphs shifts and concatenates them without a sort or a host read."""
    from .network import _fv_index
    for d in (data_v, data_f):
        for k in ('x', 'y', 'edge_weight', 'depth_direction'):
            t = getattr(d, k, None)
            if torch.is_tensor(t):
                setattr(d, k, t.contiguous())
        d.graph().ensure_in()
    _fv_index(data_f, data_v.x.shape[0])[1].get()
    return data_v, data_f
