"""Synthetic noise for clean meshes, drawn on the MI355X (geobi_mesh_noise): what produces the ``noisy/NAME_n*.obj``
files that ``train``, ``denoise`` and ``eval`` work on, and the fresh noise per epoch of ``DualDataset(noise=...)``.

The reference has no counterpart: its dataset is an external download (README.md:7 of the reference) and its noise
generator is not in its tree.  The conventions are those of its file names (``NAME_n1 .. NAME_n3`` = noise levels
0.1 .. 0.3 of the mean edge length).

The generator is counter-based (Philox4x32-10, one counter per vertex), so a noisy mesh is a pure function of
(seed, stream id of the mesh NAME, draw, vertex index) -- the ``noise`` command, a dataset built from clean meshes and a
later ``resample`` all arrive at the same bits without sharing any state.
"""
import zlib

import numpy as np
import torch

from . import _lib as L
from . import meshin, meshprep

KINDS = ('gaussian', 'impulsive')
DIRECTIONS = ('normal', 'random')
DEFAULT_LEVELS = (0.1, 0.2, 0.3)


def stream_of(name):
    """Stable Philox stream id of a mesh name: it does not depend on what else is in the folder."""
    return zlib.crc32(name.encode()) & 0xffffffff


def parse_levels(text):
    """'0.1,0.2,0.3' -> (0.1, 0.2, 0.3).  ValueError for an empty list, an empty item, a non-number, a negative or
    non-finite level."""
    items = str(text).split(',')
    levels = []
    for item in items:
        try:
            v = float(item.strip())
        except ValueError:
            raise ValueError('noise levels %r: %r is not a number' % (text, item))
        if not np.isfinite(v) or v < 0:
            raise ValueError('noise levels %r: %r is negative or not finite' % (text, item))
        levels.append(v)
    return tuple(levels)


def noisy_name(name, k):
    """Stem of the level-``k`` (1-based) noise file of mesh ``name``: the ``NAME_n<k>`` that file_pairs globs for."""
    return '%s_n%d' % (name, k)


class NoiseOptions(object):
    """What ``DualDataset(noise=...)`` and the ``noise`` command draw with."""

    def __init__(self, levels=DEFAULT_LEVELS, kind='gaussian', direction='normal', fraction=0.3, seed=1):
        self.levels = tuple(float(v) for v in (parse_levels(levels) if isinstance(levels, str) else levels))
        self.kind, self.direction, self.fraction, self.seed = kind, direction, float(fraction), int(seed)
        if not self.levels:
            raise ValueError('noise: no levels')
        check_arguments(min(self.levels), self.kind, self.direction, self.fraction)

    @staticmethod
    def of(obj):
        """A NoiseOptions, a dict of its arguments, or None -> NoiseOptions or None."""
        if obj is None or isinstance(obj, NoiseOptions):
            return obj
        return NoiseOptions(**dict(obj))

    def draw_index(self, k, d):
        """Philox draw of level ``k`` (1-based) in resampling round ``d``: rounds never share a draw."""
        return k + len(self.levels) * int(d)


def check_arguments(level, kind, direction, fraction):
    if not level >= 0 or not np.isfinite(level):
        raise ValueError('noise level %r: must be finite and not negative' % (level,))
    if kind not in KINDS:
        raise ValueError('noise kind %r: one of %s' % (kind, ', '.join(KINDS)))
    if direction not in DIRECTIONS:
        raise ValueError('noise direction %r: one of %s' % (direction, ', '.join(DIRECTIONS)))
    if not 0.0 <= fraction <= 1.0:
        raise ValueError('noise fraction %r outside [0, 1]' % (fraction,))


class MeshGeometry(object):
    """What the noise of one clean mesh needs and no draw changes: device points and face table (range-checked), the
    vertex -> face incidence, the vertex normals and the mean edge length ``L`` (device scalar and host float)."""

    def __init__(self, points, faces, device=None):
        self.points, self.faces = meshin.device_mesh(points, faces, meshin.default_device(device))
        V = self.points.shape[0]
        self.incidence = meshprep.vertex_faces(self.faces, V)
        self.graph_v = meshprep.ring_graph(0, self.faces, self.incidence[0], self.incidence[1], V)
        self.vnormal = meshprep.mesh_normals(self.points, self.faces, self.incidence[0], self.incidence[1])[2]
        # the float32 value as patches.predict_mesh and DualDataset read it
        self.mean_edge = float(torch.tensor(meshprep.mean_edge_length(self.points, self.graph_v).tolist()[0],
                                            dtype=torch.float32))

    def sigma(self, level):
        """``level * L`` rounded once to float32: the value the kernel is handed."""
        return float(np.float32(np.float32(level) * np.float32(self.mean_edge)))

    def draw(self, level, kind='gaussian', direction='normal', fraction=0.3, seed=1, stream_id=0, draw=0, out=None):
        check_arguments(level, kind, direction, fraction)
        out = torch.empty_like(self.points) if out is None else out
        mesh_noise(self.points, self.vnormal, self.sigma(level), kind, direction, fraction, seed, stream_id, draw, out)
        return out


def mesh_noise(points, vnormal, sigma, kind, direction, fraction, seed, stream_id, draw, out):
    """geobi_mesh_noise on device tensors: out[v] = points[v] + displacement(v).  ``out`` may be ``points``."""
    L.require_device(points, 'points')
    if kind not in KINDS or direction not in DIRECTIONS:
        raise ValueError('noise kind %r / direction %r' % (kind, direction))
    if points.dtype != torch.float32 or out.dtype != torch.float32 or out.shape != points.shape:
        raise ValueError('mesh_noise: float32 [V, 3] arrays of one shape')
    if not 0 <= int(seed) < 2 ** 64 or not 0 <= int(stream_id) < 2 ** 32 or not 0 <= int(draw) < 2 ** 32:
        raise ValueError('mesh_noise: seed is 64 bits, stream_id and draw are 32 bits, none negative')
    L.call('geobi_mesh_noise', L.ptr(points), L.ptr(vnormal) if direction == 'normal' else None, int(points.shape[0]),
           float(sigma), KINDS.index(kind), DIRECTIONS.index(direction), float(fraction), int(seed), int(stream_id),
           int(draw), L.ptr(out), L.stream())
    return out


def add_noise(points, faces, level, *, kind='gaussian', direction='normal', fraction=0.3, seed, stream_id=0, draw=0,
              device=None):
    """(points [V, 3], faces [F, 3]) -> noisy points, device tensor [V, 3]: every vertex displaced by
    ``sigma * g`` along its vertex normal (``direction='normal'``) or along a uniformly random direction (``'random'``),
    ``g`` standard normal, ``sigma = level * L`` with ``L`` the mean edge length of the input mesh; ``kind='impulsive'``
    moves only a ``fraction`` of the vertices.  Same (seed, stream_id, draw) -> same bits.  ValueError for a negative
    level, a fraction outside [0, 1], an unknown kind or direction; GeobiError for faces outside [0, V)."""
    check_arguments(level, kind, direction, fraction)
    return MeshGeometry(points, faces, device).draw(level, kind, direction, fraction, seed, stream_id, draw)
