"""examples/shear_layer.py through FlowSolver2d on the device, a few thousand cells: the Smagorinsky viscosity sits in the shear band,
and the VTK export carries the field."""
import glob
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shear_layer_example(hip_lib, tmp_path):
    spec = importlib.util.spec_from_file_location('shear_layer', os.path.join(ROOT, 'examples', 'shear_layer.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    inside, outside, s = mod.run(nx=48, ny=24, t_end=30.0, export=True, output_directory=str(tmp_path))
    assert s.mesh2d.num_cells == 2304
    print('inside', inside, 'outside', outside)
    assert inside > outside and inside > 1e-10
    files = sorted(glob.glob(os.path.join(str(tmp_path), 'SmagViscosity2d', 'SmagViscosity2d_*.vtu')))
    assert len(files) == 2                                               # the initial state and the end
    with open(files[-1], 'rb') as f:
        head = f.read(4096)
    assert b'Name="Smag. viscosity"' in head
