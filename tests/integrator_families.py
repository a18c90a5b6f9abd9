"""Families registered with register_family(integrator="rk4") for the tests (test infrastructure;
__graft_entry__.build() pre-builds their libraries so the GPU box only loads them).

The ODEs and the parametrised costs are the ones of tests/custom_families.py; only the
discretisation differs: one classical Runge-Kutta step per stage (noc.utils.runge_kutta) instead of
one Euler step.  Each family has its torch restatement for the autodiff oracle, whose dynamics are
oracle.problems.discretize_dynamics(ode, dt, 1).

rk4_cartpole (nx=4, nu=1): the reference cart-pole ODE (CR:54-81), whose row xdot = v has a
constant ODE Jacobian that is not a constant of the RK4 map.
rk4_actuated_pendulum (nx=3, nu=1): a KKT shape the default library does not instantiate.
rk4_vectored_cartpole (nx=4, nu=2): nonlinear in both controls, so the u-blocks of the stage
sensitivities and fuu / fxu run with NU > 1.
"""
import custom_families as CF

DT = 0.05

# the cart-pole's parametrised cost: the weights / goal / bound of custom_families' track-limit
# costs (CR:27-45) without the state constraint and the quartic term
CARTPOLE = dict(nx=4, nu=1, goal=[float(v) for v in CF._CP_GOAL], wx=[float(v) for v in CF._CP_WX],
                wu=[1e-3], wf=[float(v) for v in CF._CP_WF], u_bound=50.0, wrap_index=1)

# name -> (numpy ODE, parametrised cost)
SPECS = {"rk4_cartpole": (CF.cartpole_ode, CARTPOLE),
         "rk4_actuated_pendulum": (CF.actuated_pendulum_ode, CF.ACT_PEND),
         "rk4_vectored_cartpole": (CF.vectored_cartpole_ode, CF.VC)}


def register(name, dt=DT, build=True, integrator="rk4", verbose=False):
    """The family `name` (integrator="euler": the Euler family of the same ODE and cost, under a
    name of its own)."""
    from noc import families
    ode, spec = SPECS[name]
    reg_name = name if integrator == "rk4" else name.replace("rk4_", "euler_")
    return families.register_family(reg_name, ode, dt=dt, build=build, integrator=integrator,
                                    verbose=verbose, **spec)


def cartpole_ode_torch(state, action):
    import torch
    g, pl, mc, mp = 9.81, 0.5, 10.0, 1.0
    mt = mc + mp
    th, xd, thd = state[1], state[2], state[3]
    a = action[0]
    s, c = torch.sin(th), torch.cos(th)
    xdd = (a + mp * s * (pl * thd ** 2 + g * c)) / (mc + mp * s ** 2)
    thdd = (-a * c - mp * pl * thd ** 2 * c * s - mt * g * s) / (pl * mc + pl * mp * s ** 2)
    return torch.stack((xd, thd, xdd, thdd))


def actuated_pendulum_ode_torch(state, action):
    import torch
    g, length, damping, lag = 9.81, 1.0, 0.1, 0.05
    return torch.stack((state[1], -g / length * torch.sin(state[0]) - damping * state[1] + state[2],
                        (action[0] - state[2]) / lag))


def vectored_cartpole_ode_torch(state, action):
    import torch
    g, pl, mc, mp = CF.VC_PHYS
    th, xd, thd = state[1], state[2], state[3]
    fh = action[0] * torch.cos(CF.VC_GAIN * action[1])
    fv = action[0] * torch.sin(CF.VC_GAIN * action[1])
    s, c = torch.sin(th), torch.cos(th)
    xdd = (fh + mp * s * (pl * thd ** 2 + g * c)) / (mc + mp * s ** 2)
    thdd = (-fh * c - mp * pl * thd ** 2 * c * s - (mc + mp) * g * s + CF.VC_LEVER * fv) / (
        pl * mc + pl * mp * s ** 2)
    return torch.stack((xd, thd, xdd, thdd))


TORCH_ODES = {"rk4_cartpole": cartpole_ode_torch,
              "rk4_actuated_pendulum": actuated_pendulum_ode_torch,
              "rk4_vectored_cartpole": vectored_cartpole_ode_torch}


def torch_ocp(name, dt=DT, integrator="rk4"):
    """The same problem in torch (oracle/problems.py conventions): the reference's RK4
    discretisation of the ODE (integrator="euler": its Euler one) with the parametrised cost."""
    from oracle import problems as PR
    _, spec = SPECS[name]
    ode = TORCH_ODES[name]
    dyn = PR.discretize_dynamics(ode, dt, 1) if integrator == "rk4" else PR.euler(ode, dt)
    return PR.TorchOCP(dyn, *CF._param_cost_torch(spec, spec["wrap_index"]), spec["nx"],
                       spec["nu"], name)


def build_all(verbose=False):
    """Register (and build once) every RK4 test family; returns their OCPs."""
    return [register(name, verbose=verbose) for name in SPECS]
