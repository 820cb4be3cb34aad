"""The exactly integrated cases of tests/golden/exact_weakforms*.json.gz (written by tests/golden/make_exact_weakform_golden.py) as
meshes, numpy arrays, oracle keywords and device calls: shared by tests/test_exact_weakforms.py (CPU) and
tests/test_gpu_exact_weakforms.py (plain module, no GPU needed)."""
import glob
import gzip
import json
import os

import numpy as np

from thetis_amd import _lib
from thetis_amd.mesh import Mesh2d

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EPS = np.finfo(np.float64).eps
BND_KINDS = [('elev',), ('uv',), ('un',), ('flux',), ('elev', 'uv'), ('elev', 'un'), ('elev', 'flux')]
SOURCES = {'coriolis': ('coriolis', _lib.FIELD_CORIOLIS), 'linear_drag': ('linear_drag_coefficient', _lib.FIELD_LINEAR_DRAG),
           'atmospheric_pressure': ('atmospheric_pressure', _lib.FIELD_ATMOSPHERIC_PRESSURE),
           'momentum_source': ('momentum_source', _lib.FIELD_MOMENTUM_SOURCE), 'volume_source': ('volume_source', _lib.FIELD_VOLUME_SOURCE),
           'wind_stress': ('wind_stress', _lib.FIELD_WIND_STRESS)}
_DOCS = None


def documents():
    """{file name: parsed JSON}"""
    global _DOCS
    if _DOCS is None:
        _DOCS = {}
        for path in sorted(glob.glob(os.path.join(GOLDEN, 'exact_weakforms*.json.gz'))):
            with gzip.open(path, 'rt') as fh:
                _DOCS[os.path.basename(path)[:-3]] = json.load(fh)
    return _DOCS


def _mesh(entry):
    mesh = Mesh2d(np.array(entry['vertices'], dtype=np.float64), np.array(entry['cells']), marker_fn=None)
    assert np.array_equal(mesh.cells, np.array(entry['cells'])), 'the file lists counter-clockwise cells'
    nbr = mesh.cell_nbr.copy()
    assert (nbr < 0).sum() == len(entry['facet_markers'])
    for cell, facet, marker in entry['facet_markers']:
        assert nbr[cell, facet] < 0
        nbr[cell, facet] = -marker
    mesh.cell_nbr = np.ascontiguousarray(nbr)
    mesh.boundary_len = {int(m): float(v) for m, v in entry['boundary_len'].items()}
    computed = mesh._boundary_length()
    assert all(abs(computed[m] - v) < 1e-12*v for m, v in mesh.boundary_len.items())
    return mesh


def _unhex(pairs, shape):
    hi = np.array([float.fromhex(p[0]) for p in pairs]).reshape(shape)
    lo = np.array([float.fromhex(p[1]) for p in pairs]).reshape(shape)
    return hi, lo


class Case(object):
    """One case: ``exact[result][field] = (hi, lo)``; results 'tendency', 'step', 'two_steps' (merged over the files)"""

    def __init__(self, name, raw, mesh, entry):
        self.name, self.raw, self.mesh = name, dict(raw), mesh
        self.group = raw['group']
        self.dt = raw['dt']
        self.share = raw['share']
        self.is_tracer = 'tracer' in raw
        self.bath = np.full(mesh.num_vertices, entry['depth'])
        self.g = entry['g_grav']
        self.eta = np.array(entry['eta'])
        self.uv = np.array(entry['uv'])
        self.T = np.array(entry['tracer'])
        if self.is_tracer:
            self.uv = np.array(raw['tracer']['uv'])[mesh.cells]           # continuous P1 velocity
        self.exact = {}
        self.add_results(raw)

    def add_results(self, raw):
        n, k = self.mesh.cells.shape
        for res in ('tendency', 'step', 'two_steps'):
            if res in raw:
                self.exact[res] = {f: _unhex(v, (n, k, 2) if f == 'uv' else (n, k)) for f, v in raw[res].items()}

    # ---- values of the file as arrays
    def nodal(self, v, vec=False):
        """constant -> itself; vertex values of a P1 Function -> DG nodal array (N, k[, 2])"""
        a = np.asarray(v, dtype=np.float64)
        if a.ndim == (1 if vec else 0):
            return tuple(a) if vec else float(a)
        return a[self.mesh.cells]

    def bnd_conditions(self):
        return {int(m): {key: self.nodal(v, key == 'uv') for key, v in funcs.items()} for m, funcs in self.raw.get('bnd', {}).items()}

    def kinds(self):
        """[(sorted boundary keys, 'const' | 'field')] of the shallow-water boundary dicts"""
        out = []
        for funcs in self.raw.get('bnd', {}).values():
            fld = any(np.ndim(v) > (1 if key == 'uv' else 0) for key, v in funcs.items())
            out.append((tuple(k for k in ('elev', 'uv', 'un', 'flux') if k in funcs), 'field' if fld else 'const'))
        return out

    def oracle_kwargs(self):
        kw = dict(g=self.g, use_nonlinear_equations=False, use_lax_friedrichs_velocity=False, bnd_conditions=self.bnd_conditions())
        for key, v in self.raw.get('sources', {}).items():
            kw[SOURCES[key][0]] = np.asarray(v, dtype=np.float64) if np.ndim(v) else float(v)
        visc = self.raw.get('viscosity')
        if visc:
            nu = visc['nu']
            kw.update(horizontal_viscosity=np.asarray(nu) if np.ndim(nu) else float(nu), sipg_factor=visc['sipg_factor'],
                      use_grad_div_viscosity_term=visc['grad_div'], use_grad_depth_viscosity_term=True)
        return kw

    def ref_expected(self):
        """whether the C restatement has every option of the case (by the case's content, not by trying): constant boundary data,
        a constant drag, no viscosity; tracer: advection, Lax-Friedrichs, source and constant 'value' boundaries only"""
        if self.is_tracer:
            tc = self.raw['tracer']
            return ('diffusivity' not in tc and not tc['conservative']
                    and all(set(f) == {'value'} and not np.ndim(f['value']) for f in tc['bnd'].values()))
        return ('viscosity' not in self.raw and all(kind == 'const' for _, kind in self.kinds())
                and not np.ndim(self.raw.get('sources', {}).get('linear_drag', 0.0)))

    def ref_kwargs(self):
        """keywords of the C restatement (RefSWE)"""
        assert self.ref_expected(), self.name
        kw = dict(g=self.g, use_nonlinear_equations=False, use_lax_friedrichs_velocity=False,
                  bnd_conditions={} if self.is_tracer else self.bnd_conditions())
        for key, v in self.raw.get('sources', {}).items():
            kw[SOURCES[key][0]] = np.asarray(v, dtype=np.float64)[self.mesh.cells] if np.ndim(v) else float(v)
        return kw

    def ref_tracer_kwargs(self):
        """keywords of the C tracer restatement (RefTracer)"""
        tc = self.raw['tracer']
        return dict(use_lax_friedrichs_tracer=tc['lax_friedrichs'], source=np.asarray(tc['source'])[self.mesh.cells],
                    bnd_values={int(m): float(f['value']) for m, f in tc['bnd'].items()})

    def tracer_kwargs(self):
        tc = self.raw['tracer']
        bcs = {int(m): {key: self.nodal(v) for key, v in funcs.items()} for m, funcs in tc['bnd'].items()}
        kw = dict(conservative=tc['conservative'], use_lax_friedrichs_tracer=tc['lax_friedrichs'],
                  source=np.asarray(tc['source']), bnd_conditions=bcs)
        if 'diffusivity' in tc:
            mu = tc['diffusivity']
            kw.update(diffusivity=np.asarray(mu) if np.ndim(mu) else float(mu), sipg_factor_tracer=tc['sipg_factor'])
        return kw

    # ---- the device, through the public calls the randomised tests use
    def make_device(self, reorder='auto'):
        from thetis_amd.device import Swe2dDevice
        dev = Swe2dDevice(self.mesh, self.bath, self.dt, g_grav=self.g, use_nonlinear_equations=False,
                          use_lax_friedrichs_velocity=False, boundary_len=self.mesh.boundary_len, reorder=reorder)
        for key, v in self.raw.get('sources', {}).items():
            if np.ndim(v):
                dev.set_field(SOURCES[key][1], np.asarray(v, dtype=np.float64)[self.mesh.cells])
            else:
                assert key == 'linear_drag'
                dev.set_scalar(_lib.SCALAR_LINEAR_DRAG, float(v))
        visc = self.raw.get('viscosity')
        if visc:
            nu = visc['nu']
            dev.set_viscosity(np.asarray(nu) if np.ndim(nu) else float(nu), sipg_factor=visc['sipg_factor'],
                              use_grad_div_viscosity_term=visc['grad_div'], use_grad_depth_viscosity_term=True)
        for marker, funcs in self.bnd_conditions().items():
            dev.set_bc(marker, funcs)
        dev.set_state(self.uv, self.eta)
        return dev

    def add_device_tracer(self, dev):
        tc = self.raw['tracer']
        kw = self.tracer_kwargs()
        tid = dev.add_tracer()
        dev.tracer_set_conservative(tid, tc['conservative'])
        dev.tracer_set_options(tc['lax_friedrichs'], 1.0, 1.0)
        dev.tracer_set_source(tid, kw['source'][self.mesh.cells])
        diff = 'diffusivity' in kw
        if diff:
            dev.tracer_set_diffusivity(tid, kw['diffusivity'], tc['sipg_factor'])
        for marker, funcs in kw['bnd_conditions'].items():
            v = funcs.get('value')
            if v is not None:
                dev.tracer_set_bc(tid, marker, v)
            if diff:
                kind = 1 if 'diff_flux' in funcs else (3 if v is None else (4 if isinstance(v, np.ndarray) else 2))
                dev.tracer_set_diffusion_bc(tid, marker, kind, funcs.get('diff_flux', 0.0))
        dev.tracer_set_state(tid, self.T)
        return tid


_CASES = None


def cases():
    """{name: Case}, meshes shared between the cases of a mesh"""
    global _CASES
    if _CASES is None:
        _CASES, meshes = {}, {}
        for doc in documents().values():
            for mname, entry in doc['meshes'].items():
                if mname not in meshes:
                    meshes[mname] = _mesh(entry)
                entry = dict(entry, depth=doc['depth'], g_grav=doc['g_grav'])
                for name, raw in doc['cases'].items():
                    if name in _CASES:
                        _CASES[name].add_results(raw)
                    else:
                        _CASES[name] = Case(name, raw, meshes[mname], entry)
    return _CASES


def rel_err(computed, exact):
    """relative inf-norm error against the correctly rounded exact values (what the project's bounds are stated in)"""
    hi = exact[0]
    return float(np.abs(computed - hi).max()/np.abs(hi).max())


def eps_units(computed, exact):
    """inf-norm error against hi + lo in units of eps*max|exact|"""
    hi, lo = exact
    return float(np.abs((computed - hi) - lo).max()/(EPS*np.abs(hi).max()))
