"""What tests/test_gpu_filter.py and tests/test_gpu_gnf.py share: the sweep counts and fan valences, the builders of the small
meshes, the bar against the fp64 models, the noisy sphere with its ground truth, and the device inputs both filters take."""
import numpy as np
import torch

import geom_model as G

U = 2.0 ** -24
SWEEPS = (0, 1, 2, 5)
FAN_VALENCES = (3, 4, 5, 8, 9, 16, 17, 33, 64, 65, 200)


def _one_face():
    return G._f32_values([[0.1, 0.2, 0.3], [1.3, 0.1, 0.2], [0.4, 1.1, 0.9]]), torch.tensor([[0, 1, 2]])


def _icosahedron():
    from geobi_gnn_amd import meshgen
    pts, faces = meshgen.icosphere(1)
    return G._f32_values(pts), torch.from_numpy(np.asarray(faces, dtype=np.int64))


def _all_degenerate():
    """Collinear points: every face has exactly zero area, the centroids differ."""
    pts = G._f32_values([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0], [4.0, 0.0, 0.0]])
    return pts, torch.tensor([[0, 1, 2], [1, 2, 3], [0, 0, 3]])


def _opposite():
    """One triangle with both orientations: equal areas, one centroid, exactly opposite normals."""
    return G._f32_values([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), torch.tensor([[0, 1, 2], [0, 2, 1]])


def _shifted():
    pts, faces = G.sphere(8, 0.3, 1)
    return G._f32_values((pts + torch.tensor([1000.0, -2000.0, 500.0], dtype=torch.float64)).numpy()), faces


FANS = {'fan%d' % v: (lambda v_=v: G.fan(v_)) for v in FAN_VALENCES}


def _bar(d32):
    return 8 * max(d32, 4 * U)


def _sphere8_with_truth():
    from geobi_gnn_amd import meshgen
    noisy, clean, faces = meshgen.noisy_icosphere(8, 0.3, seed=1)
    return noisy, clean, np.asarray(faces, dtype=np.int64)


def _angle(a, b):
    return float(G.row_terms(a, b, 3).mean())


class _DeviceMesh(object):
    """A filter's device inputs for one mesh: records, facet graph, the spatial scale."""

    def __init__(self, pts, faces, dev, sigma_s=1.0):
        from geobi_gnn_amd import filters, meshprep
        self.filters = filters
        self.pts = pts.float().to(dev).contiguous()
        self.fv = faces.to(device=dev, dtype=torch.int32).contiguous()
        rowptr, lst = meshprep.vertex_faces(self.fv, self.pts.shape[0])
        self.graph = meshprep.ring_graph(1, self.fv, rowptr, lst, self.fv.shape[0])
        self.rec_c, self.rec_n = filters.face_records(self.pts, self.fv)
        self.inv2ss = filters.spatial_scale(self.pts, self.fv, self.graph, sigma_s)
