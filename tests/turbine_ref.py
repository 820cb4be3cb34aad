"""
Independent numpy statement of the tidal turbine terms, written from the reference's formulas:

  thrust / power table          thetis/turbines.py:109-145   (0 below speeds[0], linear between entries, 0 from speeds[-1] on)
  thrust area, alpha, c_t       thetis/turbines.py:36-58
  TurbineDragTerm               thetis/shallowwater_eq.py:783-791   f = c_t d |u| u.psi / H dx(farm), residual -f, no norm_smoother
  power                         thetis/turbines.py:85-93, 167-168, depth = the static bathymetry (:233, :252)

Quadrature rule and mass inverse are the oracle's (``oracle.swe2d_oracle.SWEOracle.cell_quad`` / ``solve_mass``); nothing of
thetis_amd is imported here.  A farm is a dict: diameter, projected_diameter, C_support, A_support, upwind (bool), and either
thrust / power (constant type) or speeds, thrust_table, power_table; density (N, k) nodal, zero outside the farm.
"""
import numpy as np

RHO0 = 1000.0


def table(speeds, values, s):
    """numpy.interp inside [speeds[0], speeds[-1]), zero outside (turbines.py:141: below cut-in 0; :123-125: from the last speed on 0)"""
    s = np.asarray(s, dtype=np.float64)
    return np.where((s >= speeds[0]) & (s < speeds[-1]), np.interp(s, speeds, values), 0.0)


def default_power_coefficient(c_t):
    return 0.5*c_t*(1 + (1 - c_t)**0.5)                        # turbines.py:100, :132


def rotor_area(farm):
    return np.pi*farm['diameter']**2/4


def thrust_area(farm, speed):
    c_t = table(farm['speeds'], farm['thrust_table'], speed) if 'speeds' in farm else farm['thrust']
    return c_t*rotor_area(farm) + farm.get('C_support', 0.0)*farm.get('A_support', 0.0)


def alpha(farm, speed, depth):
    if not farm.get('upwind', False):
        return np.ones_like(np.asarray(speed, dtype=np.float64))
    d_proj = farm.get('projected_diameter') or farm['diameter']
    return 0.5*(1 + np.sqrt(1 - thrust_area(farm, speed)/(d_proj*depth)))


def c_t(farm, speed, depth):
    return thrust_area(farm, speed)/2./alpha(farm, speed, depth)**2


def power_coefficient(farm, speed):
    if 'speeds' in farm:
        cp = farm.get('power_table') or [default_power_coefficient(c) for c in farm['thrust_table']]
        return table(farm['speeds'], cp, speed)
    return farm.get('power') or default_power_coefficient(farm['thrust'])


def drag_residual(orc, farms, uv, eta):
    """(N, k, 2): the farms' contribution to the momentum residual, -sum_farms int c_t d |u| u phi_i / H dx"""
    r = np.zeros(uv.shape)
    H = orc.nodal_depth(eta)
    for phi, _, wA in orc.cell_quad:
        u_q = np.einsum('nic,i->nc', uv, phi)
        H_q = H @ phi
        speed = np.sqrt(u_q[:, 0]**2 + u_q[:, 1]**2)
        for farm in farms:
            d_q = farm['density'] @ phi
            with np.errstate(invalid='ignore'):
                coef = np.where(d_q != 0.0, c_t(farm, speed, H_q)*d_q*speed/H_q, 0.0)
            for i in range(uv.shape[1]):
                for c in range(2):
                    r[:, i, c] -= wA*coef*phi[i]*u_q[:, c]
    return r


def drag_tendency(orc, farms, uv, eta, dt):
    """M^-1 dt F_turbine (N, k, 2)"""
    k_u, _ = orc.solve_mass(dt*drag_residual(orc, farms, uv, eta), np.zeros(eta.shape))
    return k_u


def power(orc, farm, uv, rho0=RHO0):
    """int 0.5 rho0 A_T C_P(u3^(1/3)) u3 d dx, u3 = |u|^3 / alpha^3, alpha with the static bathymetry"""
    total = 0.0
    for phi, _, wA in orc.cell_quad:
        u_q = np.einsum('nic,i->nc', uv, phi)
        h_q = orc.h @ phi
        d_q = farm['density'] @ phi
        speed = np.sqrt(u_q[:, 0]**2 + u_q[:, 1]**2)
        u3 = speed**3/alpha(farm, speed, h_q)**3
        p = 0.5*rho0*rotor_area(farm)*power_coefficient(farm, np.cbrt(u3))*u3
        total += float(np.sum((wA*p*d_q)[d_q != 0.0]))
    return total


def number_of_turbines(orc, farm):
    return float(sum(np.sum(wA*(farm['density'] @ phi)) for phi, _, wA in orc.cell_quad))
