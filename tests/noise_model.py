"""Host model of geobi_mesh_noise: Philox4x32-10 in numpy integers and the displacement in fp64.  The reference of the GPU
tests (tests/test_gpu_noise.py); its generator is pinned by the known answers in tests/test_meshnoise_host.py."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57             # Random123 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85             # Weyl key increments
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of 32-bit words, key: 2 -> 4 uint64 arrays holding the 32-bit output words."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & np.uint64(MASK) for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]            # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def uniform(words):
    """u = ((w >> 9) + 0.5) * 2^-23: exact in fp32 and in fp64, inside (0, 1)."""
    return ((np.asarray(words, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def words_of(rows, seed, stream_id, draw, block):
    key = (int(seed) & MASK, (int(seed) >> 32) & MASK)
    return philox4x32_10((np.asarray(rows, dtype=np.uint64), stream_id, draw, block), key)


def normals4(rows, seed, stream_id, draw):
    """-> dict(g [V, 4], r [V, 2] radii, cs [V, 4] = (cos, sin, cos, sin)) of block 0 in fp64."""
    u = [uniform(w) for w in words_of(rows, seed, stream_id, draw, 0)]
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    t0, t1 = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    cs = np.stack([np.cos(t0), np.sin(t0), np.cos(t1), np.sin(t1)], 1)
    r = np.stack([r0, r1], 1)
    g = np.stack([r0 * cs[:, 0], r0 * cs[:, 1], r1 * cs[:, 2], r1 * cs[:, 3]], 1)
    return {'g': g, 'r': r, 'cs': cs}


def coin(rows, seed, stream_id, draw):
    """The impulsive kind's uniform: block 1, word 0."""
    return uniform(words_of(rows, seed, stream_id, draw, 1)[0])


def displacement(rows, vnormal, sigma, kind, direction, fraction, seed, stream_id, draw):
    """fp64 displacement [V, 3] of the rows (vertex indices of the call) -> (disp, moved mask, normals4 dict).
    sigma and fraction are taken as the float32 values the kernel is handed; vnormal as its float32 rows."""
    rows = np.asarray(rows)
    n4 = normals4(rows, seed, stream_id, draw)
    g = n4['g']
    sigma = float(np.float32(sigma))
    if direction == 0:
        d = sigma * g[:, :1] * np.asarray(vnormal, dtype=np.float64)
    else:
        length = np.sqrt((g[:, 1:] ** 2).sum(1, keepdims=True))
        unit = np.where(length > 0, g[:, 1:] / np.where(length > 0, length, 1.0), np.array([[0.0, 0.0, 1.0]]))
        d = sigma * g[:, :1] * unit
    moved = np.ones(rows.shape[0], dtype=bool)
    if kind == 1:
        moved = coin(rows, seed, stream_id, draw) < float(np.float32(fraction))
    if sigma == 0.0:
        moved[:] = False
    return np.where(moved[:, None], d, 0.0), moved, n4
