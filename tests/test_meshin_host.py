"""geobi_gnn_amd.meshin on the host (no GPU): the range check of a face table as it arrives -- lists, arrays, tensors, the
int64 ids that a conversion to int32 would wrap into range --, the conversion that makes no copy, and device_mesh's shape
errors, which come before any device is asked for."""
import numpy as np
import pytest
import torch

from geobi_gnn_amd import meshin
from geobi_gnn_amd._lib import GeobiError

FACES = [[0, 1, 2], [1, 2, 3]]                   # of a mesh of 4 vertices
POINTS = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], dtype=np.float32)


@pytest.mark.parametrize('form', [list, lambda f: np.array(f, dtype=np.int32), lambda f: np.array(f, dtype=np.int64),
                                  torch.tensor, lambda f: torch.tensor(f, dtype=torch.int32)],
                         ids=['list', 'int32', 'int64', 'tensor', 'tensor32'])
def test_check_faces_passes_a_table_in_range(form):
    assert meshin.check_faces(form(FACES), 4) is None
    with pytest.raises(GeobiError, match=r'faces index vertices outside \[0, 3\)'):
        meshin.check_faces(form(FACES), 3)


def test_check_faces_passes_an_empty_table():
    for empty in ([], np.zeros((0, 3), dtype=np.int64), torch.zeros((0, 3), dtype=torch.int32)):
        meshin.check_faces(empty, 4)
        meshin.check_faces(empty, 0)


@pytest.mark.parametrize('bad', [4, -1, 2 ** 32 + 1, -2 ** 32 + 2])
def test_check_faces_refuses_an_id_outside(bad):
    """V and -1, and the two int64 ids that torch's conversion to int32 turns into 1 and 2: checked as they arrive."""
    table = np.array([[0, 1, 2], [1, bad, 3]], dtype=np.int64)
    for t in (table, table.tolist(), torch.from_numpy(table)):
        with pytest.raises(GeobiError, match=r'^faces index vertices outside \[0, 4\)$'):
            meshin.check_faces(t, 4)
        with pytest.raises(ValueError, match=r'^clean_mesh: faces index vertices outside \[0, 4\)$'):
            meshin.check_faces(t, 4, what='clean_mesh: faces', error=ValueError)
        with pytest.raises(GeobiError, match=r'^fv_indices index vertices outside \[0, 4\)$'):
            meshin.check_faces(t, 4, 'fv_indices')
    assert not issubclass(GeobiError, ValueError)


def test_to_device_returns_a_fitting_tensor_itself():
    t = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    assert meshin.to_device(t, 'cpu', torch.float32) is t
    assert meshin.as_tensor(t) is t
    f = torch.tensor(FACES, dtype=torch.int32)
    assert meshin.to_device(f, torch.device('cpu'), torch.int32) is f
    # what does not fit is converted: dtype, layout, lists and arrays
    g = meshin.to_device(torch.tensor(FACES), 'cpu', torch.int32)
    assert g.dtype == torch.int32 and g.tolist() == FACES
    cut = meshin.to_device(t[:, :2], 'cpu', torch.float32)
    assert cut.is_contiguous() and torch.equal(cut, t[:, :2])
    for a in (POINTS, POINTS.tolist(), POINTS.astype(np.float64)):
        p = meshin.to_device(a, 'cpu', torch.float32)
        assert p.dtype == torch.float32 and p.is_contiguous() and np.array_equal(p.numpy(), POINTS)


@pytest.mark.parametrize('points,faces', [(POINTS[:, :2], FACES), (POINTS.reshape(-1), FACES), (POINTS, [0, 1, 2, 1, 2, 3]),
                                          (POINTS, [[0, 1, 2, 3]]), (POINTS, [])])
def test_device_mesh_shape_errors(points, faces):
    with pytest.raises(ValueError, match=r'points \[V,3\] and faces \[F,3\] expected'):
        meshin.device_mesh(points, faces)


def test_there_is_no_cpu_fallback():
    with pytest.raises(GeobiError, match='no CPU fallback'):
        meshin.device_mesh(POINTS, FACES, device='cpu')
    with pytest.raises(GeobiError, match='no CPU fallback'):
        meshin.default_device('cpu')
