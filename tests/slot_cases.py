"""The meshes of tests/test_tile_slots.py (the staging-slot sources of the two-ring tiles, on the host) and of
tests/test_gpu_fuse3_slots.py (the three-stage kernel that gathers by them, against the stage launches).  No GPU, no library."""
import numpy as np

import tile_cases
from helpers import channel_case, delaunay_case

# Delaunay triangulation of 1000 random points (helpers.delaunay_case): 2 122 triangles; its tiles are runs of a Hilbert order.  With the
# curve of level 16 (ordering.hilbert_cell_order's default) the runs are compact and no tile of such a mesh has more than ~80 staging
# slots; the curve of level 2 (4 x 4 boxes, the cells of a box in the mesh's numbering) cuts ragged tiles whose second ring is long:
# at this seed one of 24 tiles has 138 slots (tests/test_tile_slots.py asserts > 128) - more than two waves' worth of lanes
DELAUNAY = dict(n_points=1000, lx=10e3, ly=6e3, seed=1)
HILBERT_LEVEL = 2


def rectangle(nx, ny, seed=19):
    return channel_case(nx=nx, ny=ny, lx=100e3, ly=60e3, seed=seed, amp_eta=0.3, amp_u=0.2)


def delaunay():
    return delaunay_case(**DELAUNAY)


def coarse_hilbert_order(mesh):
    from thetis_amd import ordering
    return ordering.hilbert_cell_order(np.asarray(mesh.vertex_xy)[np.asarray(mesh.cells)].mean(axis=1), order=HILBERT_LEVEL)


def tilings():
    """name -> (mesh, bath, uv, eta, setup) with setup(dev) = the tile order handed to a device, or None: the library's own tiles"""
    from thetis_amd import ordering
    out = {}
    small = rectangle(3, 2)
    out['tri3x2'] = small + (None,)
    case = rectangle(23, 17)
    for px, py in ((11, 8), (5, 3)):
        order = ordering.triple_tile_order(case[0], px, py)
        out['tri23x17_patches{}x{}'.format(px, py)] = case + ((lambda dev, o=order: dev.fused_set_triple_tiles(*o)),)
    dl = delaunay()
    horder = coarse_hilbert_order(dl[0])
    out['delaunay_hilbert'] = dl + ((lambda dev, o=horder: dev.fused_set_order(o)),)
    return out


def builder_case(name):
    """the case of ``name`` as tile_cases.write_builder_input takes it"""
    from thetis_amd import ordering
    if name == 'tri3x2':
        return tile_cases._case(rectangle(3, 2)[0], ('triple',))
    if name.startswith('tri23x17_patches'):
        px, py = (int(x) for x in name[len('tri23x17_patches'):].split('x'))
        mesh = rectangle(23, 17)[0]
        return tile_cases._case(mesh, ('triple',), triple=ordering.triple_tile_order(mesh, px, py))
    assert name == 'delaunay_hilbert'
    mesh = delaunay()[0]
    return tile_cases._case(mesh, ('triple',), order=coarse_hilbert_order(mesh))


NAMES = ['tri3x2', 'tri23x17_patches11x8', 'tri23x17_patches5x3', 'delaunay_hilbert']
