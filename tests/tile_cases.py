"""The meshes and tile orders of tests/golden/tile_tables.json, as the tile-table builder (thetis_amd/csrc/swe2d_tiles.h) gets them:
packed neighbour codes in the device numbering, the order and the tile starts.  Shared by tests/test_tile_tables.py (the builder by
itself, on the host) and tests/test_gpu_tile_tables.py (the counts the compiled library reports).  No GPU, no library."""
import os

import numpy as np

COAST = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coast.msh')


def device_numbering(mesh, n_owned=None, ranges=None):
    """(perm, inv_perm, neighbours, neighbour facets) in the device numbering of ``Swe2dDevice(mesh, ..., reorder='auto')``:
    perm[i_device] = i_caller, boundary facets = -slot of the marker"""
    from thetis_amd import ordering
    n = int(np.asarray(mesh.cells).shape[0])
    n_owned = n if n_owned is None else int(n_owned)
    nbr0 = np.asarray(mesh.cell_nbr).astype(np.int64)
    nbf0 = np.asarray(mesh.cell_nbr_facet)
    markers = sorted(int(m) for m in np.unique(-nbr0[nbr0 < 0]))
    lut = np.zeros(max(markers) + 1, dtype=np.int64)
    lut[markers] = 1 + np.arange(len(markers))
    nbr0 = np.where(nbr0 < 0, -lut[np.where(nbr0 < 0, -nbr0, 0)], nbr0)
    bounds = sorted(set([0] + [int(b) for b in (ranges or (n_owned,))] + [n]))
    perm = np.arange(n)
    for a, b in zip(bounds[:-1], bounds[1:]):
        if b - a > 1 and a < n_owned:
            perm[a:b] = a + ordering.auto_cell_order(mesh, a, b)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(n)
    nb = nbr0[perm]
    nb[nb >= 0] = inv[nb[nb >= 0]]
    return perm, inv, nb, nbf0[perm].astype(np.int64)


def packed_codes(nb, nbf):
    """[facet][stride] int32 as swe2d_create packs them: (neighbour << 2) | its facet, or -marker; the stride a multiple of 64"""
    n, k = nb.shape
    stride = -(-n//64)*64
    out = np.zeros((k, stride), dtype=np.int32)
    out[:, :n] = np.where(nb >= 0, (nb << 2) | nbf, nb).T
    return out


def _case(mesh, kinds, order=None, triple=None, n_owned=None, ranges=None):
    """order: the caller's fused_set_order; triple: the caller's (order, starts) of fused_set_triple_tiles"""
    perm, inv, nb, nbf = device_numbering(mesh, n_owned, ranges)
    c = {'mesh': mesh, 'kinds': kinds, 'nbr': nb, 'codes': packed_codes(nb, nbf), 'caller_order': order, 'caller_triple': triple}
    c['order'] = None if order is None else inv[np.asarray(order)].astype(np.int32)
    c['triple_order'] = c['triple_start'] = None
    if triple is not None:
        start = np.zeros(len(perm), dtype=np.int32)
        start[np.asarray(triple[1])] = 1
        c['triple_order'], c['triple_start'] = inv[np.asarray(triple[0])].astype(np.int32), start
    return c


def builder_input(c, kind):
    """(order, start) that ``kind`` ('pair' | 'quad' | 'triple') of case ``c`` is built from: the two-ring tiles take their own order
    where there is one, else the pair's"""
    if kind == 'triple' and c['triple_order'] is not None:
        return c['triple_order'], c['triple_start']
    return c['order'], None


def hilbert_order(mesh):
    from thetis_amd import ordering
    return ordering.hilbert_cell_order(np.asarray(mesh.vertex_xy)[np.asarray(mesh.cells)].mean(axis=1))


_CASES = {}


def cases():
    """name -> case; built once"""
    if _CASES:
        return _CASES
    from thetis_amd import ordering
    from thetis_amd.mesh import RectangleMesh
    from thetis_amd.meshio import read_gmsh
    from thetis_amd.partition import build_partition, strip_owner
    tri = RectangleMesh(24, 16, 100e3, 50e3)
    both = ('pair', 'triple')
    _CASES['tri24x16'] = _case(tri, both)
    _CASES['tri24x16_patches11x8'] = _case(tri, ('triple',), triple=ordering.triple_tile_order(tri, 11, 8))
    _CASES['tri24x16_patches6x4'] = _case(tri, ('triple',), triple=ordering.triple_tile_order(tri, 6, 4))
    _CASES['tri24x16_hilbert'] = _case(tri, both, order=hilbert_order(tri))
    _CASES['tri29x13'] = _case(RectangleMesh(29, 13, 100e3, 50e3), both)
    _CASES['coast'] = _case(read_gmsh(COAST), both)
    part = build_partition(tri, strip_owner(tri, 2), 0)
    _CASES['tri24x16_rank0of2'] = _case(part, both, order=ordering.fused_tile_order(part), triple=ordering.triple_tile_order(part, 11, 8),
                                        n_owned=part.n_owned, ranges=part.reorder_ranges())
    quad = RectangleMesh(25, 16, 100e3, 50e3, quadrilateral=True)
    _CASES['quad25x16'] = _case(quad, ('quad',))
    _CASES['quad25x16_hilbert'] = _case(quad, ('quad',), order=hilbert_order(quad))
    return _CASES


def write_builder_input(path, c, kind):
    order, start = builder_input(c, kind)
    k, stride = c['codes'].shape
    n = c['nbr'].shape[0]
    parts = [np.array([k, stride, n, order is not None, start is not None], dtype=np.int32), c['codes'].ravel()]
    parts += [a for a in (order, start) if a is not None]
    np.concatenate(parts).astype(np.int32).tofile(path)


def rot_of_tile(tile):
    """SWE_FUSE3_ROT of swe2d_tiles.h: the top two bits of tile x 2^32/phi"""
    return ((tile*0x9E3779B1) & 0xffffffff) >> 30


def device_stream(kind, t):
    """the int32 stream of the device tables (records, then counts) as swe2d_api_fuse.hip packs them from a table ``t`` (dict of arrays):
    int2 {cell, w0 | w1 << 10 | w2 << 20}, quadrilaterals int4 {cell, w0..2, w3, 0}; counts n_inner, two-ring tiles int2 {n_inner, n_mid | rot << 16}"""
    f = t['facet'].astype(np.int64)
    w = f[:, 0] | (f[:, 1] << 10) | (f[:, 2] << 20)
    cols = [t['cell'], w] + ([f[:, 3], np.zeros_like(w)] if kind == 'quad' else [])
    counts = np.stack([t['n_inner'], t['n_mid'] | (t['rot'] << 16)], axis=1) if kind == 'triple' else t['n_inner']
    return np.concatenate([np.stack(cols, axis=1).ravel(), np.asarray(counts).ravel()]).astype(np.int32)
