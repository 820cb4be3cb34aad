"""
Descriptor of the 2D shallow water equations for the device path.

In the reference ``ShallowWaterEquations`` (thetis/shallowwater_eq.py:893-928) is a bag of UFL terms; the terms
themselves are symbolic and Firedrake turns them into kernels.  Here the terms *are* the HIP stage kernel
(thetis_amd/csrc/swe2d_kernels.h), so this class only records which of them are switched on and checks that the
configuration is one the kernel implements:

  ExternalPressureGradientTerm :335   HUDivTerm :396   HorizontalAdvectionTerm :453 (+ Lax-Friedrichs)
  CoriolisTerm :619   AtmosphericPressureTerm :652   QuadraticDragTerm :666 (constant C_D or Manning)
  LinearDragTerm :728   MomentumSourceTerm :794   ContinuitySourceTerm :814   WindStressTerm :637   BoundaryDragTerm :704
  TurbineDragTerm :765 (tidal turbine farms on cell subdomains, thetis_amd/turbines.py)
  HorizontalViscosityTerm :513 (SIPG; separate pass kernels csrc/swe2d_sipg.h, Constant or CG-P1 viscosity)
  boundary conditions 'elev' / 'uv' / 'un' / 'flux' with constant values (get_bnd_functions :232-272)
"""
from .function import Function
from .options import Constant

__all__ = ['ShallowWaterEquations', 'DepthExpression', 'g_grav', 'rho_0', 'physical_constants']

# thetis/physical_constants.py:6-11: Constants, so that tests can re-assign them (test/swe2d/test_rossby_wave.py:154-155)
physical_constants = {'g_grav': Constant(9.81), 'rho0': Constant(1000.0), 'von_karman': Constant(0.4), 'rho_air': Constant(1.22)}
g_grav = physical_constants['g_grav']
rho_0 = physical_constants['rho0']


class DepthExpression(object):
    """Total depth options (thetis/utility.py:936-996): H = h (linear), h + eta (nonlinear)."""

    def __init__(self, bathymetry_2d, use_nonlinear_equations=True, use_wetting_and_drying=False,
                 wetting_and_drying_alpha=0.5):
        self.bathymetry_2d = bathymetry_2d
        self.use_nonlinear_equations = use_nonlinear_equations
        self.use_wetting_and_drying = use_wetting_and_drying
        self.wetting_and_drying_alpha = wetting_and_drying_alpha


class ShallowWaterEquations(object):
    SUPPORTED_TERMS = ('ExternalPressureGradientTerm', 'HorizontalAdvectionTerm', 'CoriolisTerm',
                       'AtmosphericPressureTerm', 'QuadraticDragTerm', 'LinearDragTerm', 'MomentumSourceTerm',
                       'HUDivTerm', 'ContinuitySourceTerm', 'WindStressTerm', 'BoundaryDragTerm',
                       'HorizontalViscosityTerm', 'TurbineDragTerm')

    def __init__(self, function_space, depth, options, tidal_farms=None):
        self.function_space = function_space
        self.mesh = function_space.mesh()
        self.depth = depth
        self.options = options
        # TurbineDragTerm (shallowwater_eq.py:765-791): part of the stage kernels' source-term code (csrc/swe2d_kernels.h: swe_farm_terms)
        self.tidal_farms = tidal_farms
        if options.element_family != 'dg-dg' or options.polynomial_degree != 1:
            raise NotImplementedError("the device path implements element_family='dg-dg', polynomial_degree=1 only "
                                      "(got {!r}, degree {:})".format(options.element_family, options.polynomial_degree))
        if depth.use_wetting_and_drying and not options.use_nonlinear_equations:
            raise Exception('use_wetting_and_drying needs use_nonlinear_equations')
        # NOTE with use_wetting_and_drying the reference's mass_term(TrialFunction) is not bilinear (shallowwater_eq.py:
        # 917-920, rungekutta.py:900), i.e. the reference cannot run SSPRK33 with it.  The device path
        # runs this build's own explicit formulation of the same displaced depth: nodally
        # interpolated D = (H + sqrt(H^2 + alpha^2))/2, continuity advanced in zeta = D - h.

    def check_fields(self, fields):
        """Raise for coefficients whose terms the kernel does not implement (never silently ignore physics)."""
        nu = fields.get('viscosity_h')
        if nu is not None:
            # HorizontalViscosityTerm (SIPG, shallowwater_eq.py:554-616): swe_sipg_kernel<2> / swe_sipg_kernel_quad<2>
            if isinstance(nu, Function) and nu.function_space().family != 'CG':
                raise NotImplementedError('horizontal_viscosity must be a Constant or a continuous (CG-P1) Function')
        if fields.get('quadratic_drag_coefficient') is not None and fields.get('manning_drag_coefficient') is not None:
            raise Exception('Cannot set both dimensionless and Manning drag parameter')
        if fields.get('nikuradse_bed_roughness') is not None:          # shallowwater_eq.py:692-696
            if fields.get('manning_drag_coefficient') is not None:
                raise Exception('Cannot set both Nikuradse drag and Manning drag parameter')
            if fields.get('quadratic_drag_coefficient') is not None:
                raise Exception('Cannot set both dimensionless and Nikuradse drag parameter')
        # drag coefficients may be Constants or (spatially varying) Functions: nodal fields on the device
