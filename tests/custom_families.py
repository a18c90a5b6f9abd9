"""User problem families registered through noc.families.register_family for the tests (test
infrastructure; __graft_entry__.build() pre-builds their libraries so the GPU box only loads
them).  Written with numpy exactly like the reference examples' dynamics (PR:59-72), and
restated independently in torch for the autodiff oracle (oracle/problems.py style).

actuated_pendulum (nx=3, nu=1, continuous ODE + Euler): the reference pendulum driven through a
first-order actuator, state (angle, angular velocity, torque), the command u the torque set-point;
a (3, 1) KKT shape the default library does not instantiate.

cartpole_track_limit (nx=4, nu=1): cart-pole with its own traced costs and a state constraint
(see below).

Three families with more than one control (tests/multi_control_cases.py has their 50-digit
restatement; see the sections below):
vectored_cartpole (nx=4, nu=2, parametrised cost), reaction_pendulum (nx=3, nu=2, traced costs
with a coupled control constraint and a state constraint) and triple_drive_pendulum (nx=2, nu=3,
parametrised cost, more controls than states).
"""
import math

import numpy as np

ACT_PEND = dict(nx=3, nu=1, goal=[math.pi, 0.0, 0.0], wx=[1e0, 1e-1, 1e-2], wu=[1e-3],
                wf=[1e0, 1e-1, 1e-2], u_bound=5.0, wrap_index=0)


def actuated_pendulum_ode(state, action):
    g, length, damping, lag = 9.81, 1.0, 0.1, 0.05
    angle, velocity, torque = state
    a = np.atleast_1d(action)[0]
    return np.hstack((velocity, -g / length * np.sin(angle) - damping * velocity + torque,
                      (a - torque) / lag))


def actuated_pendulum(dt, build=True):
    from noc import families
    return families.register_family("actuated_pendulum", actuated_pendulum_ode, dt=dt,
                                    build=build, **ACT_PEND)


def actuated_pendulum_torch(dt):
    """The same problem restated in torch (oracle/problems.py conventions) for torch.func."""
    import torch
    from oracle import problems as PR
    goal = torch.tensor(ACT_PEND["goal"])
    Wx = torch.diag(torch.tensor(ACT_PEND["wx"]))
    Wf = torch.diag(torch.tensor(ACT_PEND["wf"]))
    Wu = torch.diag(torch.tensor(ACT_PEND["wu"]))
    ub = ACT_PEND["u_bound"]

    def constraints(state, control):
        return torch.cat((control - ub, -control - ub))

    def err(state):
        return torch.stack((PR.wrap_angle(state[0]), state[1], state[2])) - goal

    def final_cost(state):
        e = err(state)
        return 0.5 * e @ Wf @ e

    def stage_cost(state, action, bp):
        e = err(state)
        c = 0.5 * e @ Wx @ e + 0.5 * action @ Wu @ action
        return c - bp * torch.sum(torch.log(-constraints(state, action)))

    def total_cost(states, controls, bp):
        ct = torch.func.vmap(stage_cost, in_dims=(0, 0, None))(states[:-1], controls, bp)
        return final_cost(states[-1]) + torch.sum(ct)

    def ode(state, action):
        g, length, damping, lag = 9.81, 1.0, 0.1, 0.05
        return torch.stack((state[1], -g / length * torch.sin(state[0]) - damping * state[1] + state[2],
                            (action[0] - state[2]) / lag))

    return PR.TorchOCP(PR.euler(ode, dt), constraints, stage_cost, final_cost, total_cost, 3, 1,
                       "actuated_pendulum")


# ------------------------------------------------------------------------------------------------
# cartpole_track_limit (nx=4, nu=1): the reference cart-pole ODE (CR:54-81) with the reference
# OCP's own kind of callables instead of the parametrised cost -- a STATE constraint (the cart
# stays within |x| <= X_LIMIT, besides |u| <= 50) inside the log barrier, and a non-quadratic
# stage cost (a quartic penalty on the pole rate on top of the quadratic tracking), written with
# numpy exactly like CR:18-51 writes them with jnp.  Registered through
# register_family(stage_cost=..., final_cost=..., constraints=...): traced and differentiated
# symbolically for the device.
X_LIMIT = 0.5
_CP_WX = np.array([1e0, 1e1, 1e-1, 1e-1])
_CP_WF = np.array([1e0, 1e1, 1e-1, 1e-1])
_CP_GOAL = np.array([0.0, math.pi, 0.0, 0.0])


def cartpole_ode(state, action):
    g, pl, mc, mp = 9.81, 0.5, 10.0, 1.0
    mt = mc + mp
    _, th, xd, thd = state
    a = np.atleast_1d(action)[0]
    s, c = np.sin(th), np.cos(th)
    xdd = (a + mp * s * (pl * thd ** 2 + g * c)) / (mc + mp * s ** 2)
    thdd = (-a * c - mp * pl * thd ** 2 * c * s - mt * g * s) / (pl * mc + pl * mp * s ** 2)
    return np.hstack((xd, thd, xdd, thdd))


def track_limit_constraints(state, action):
    u = np.atleast_1d(action)
    return np.hstack((u - 50.0, -u - 50.0, state[0] - X_LIMIT, -state[0] - X_LIMIT))


def _cp_err(state):
    return np.hstack((state[0], state[1] % (2.0 * np.pi), state[2], state[3])) - _CP_GOAL


def track_limit_final_cost(state):
    e = _cp_err(state)
    return 0.5 * e @ np.diag(_CP_WF) @ e


def track_limit_stage_cost(state, action, bp):
    e = _cp_err(state)
    u = np.atleast_1d(action)
    c = 0.5 * e @ np.diag(_CP_WX) @ e + 0.5 * 1e-3 * u @ u + 1e-3 * state[3] ** 4
    return c - bp * np.sum(np.log(-track_limit_constraints(state, action)))


def cartpole_track_limit(dt, build=True):
    from noc import families
    return families.register_family("cartpole_track_limit", cartpole_ode, nx=4, nu=1, dt=dt,
                                    stage_cost=track_limit_stage_cost,
                                    final_cost=track_limit_final_cost,
                                    constraints=track_limit_constraints, build=build)


def cartpole_track_limit_torch(dt):
    """The same problem restated in torch (oracle/problems.py conventions) for torch.func."""
    import torch
    from oracle import problems as PR
    goal = torch.tensor(_CP_GOAL)
    Wx, Wf = torch.diag(torch.tensor(_CP_WX)), torch.diag(torch.tensor(_CP_WF))

    def constraints(state, control):
        return torch.cat((control - 50.0, -control - 50.0, state[:1] - X_LIMIT, -state[:1] - X_LIMIT))

    def err(state):
        return torch.stack((state[0], PR.wrap_angle(state[1]), state[2], state[3])) - goal

    def final_cost(state):
        e = err(state)
        return 0.5 * e @ Wf @ e

    def stage_cost(state, action, bp):
        e = err(state)
        c = 0.5 * e @ Wx @ e + 0.5 * 1e-3 * action @ action + 1e-3 * state[3] ** 4
        return c - bp * torch.sum(torch.log(-constraints(state, action)))

    def total_cost(states, controls, bp):
        ct = torch.func.vmap(stage_cost, in_dims=(0, 0, None))(states[:-1], controls, bp)
        return final_cost(states[-1]) + torch.sum(ct)

    def ode(state, action):
        g, pl, mc, mp = 9.81, 0.5, 10.0, 1.0
        mt = mc + mp
        th, xd, thd = state[1], state[2], state[3]
        a = action[0]
        s, c = torch.sin(th), torch.cos(th)
        xdd = (a + mp * s * (pl * thd ** 2 + g * c)) / (mc + mp * s ** 2)
        thdd = (-a * c - mp * pl * thd ** 2 * c * s - mt * g * s) / (pl * mc + pl * mp * s ** 2)
        return torch.stack((xd, thd, xdd, thdd))

    return PR.TorchOCP(PR.euler(ode, dt), constraints, stage_cost, final_cost, total_cost, 4, 1,
                       "cartpole_track_limit")


# ------------------------------------------------------------------------------------------------
# vectored_cartpole (nx=4, nu=2, parametrised cost): a light cart-pole pushed by a thruster of
# thrust u0 whose nozzle is turned by the angle VC_GAIN * u1: the horizontal component
# u0 cos(VC_GAIN u1) drives the cart, the vertical one u0 sin(VC_GAIN u1) acts on the pole through
# the lever VC_LEVER.  Nonlinear in both controls: fu has two different columns, fxu is non-zero in
# both control columns (the force enters divided by mc + mp sin^2), and d2 / du0 du1 is not zero.
VC = dict(nx=4, nu=2, goal=[0.0, math.pi, 0.0, 0.0], wx=[1e0, 1e1, 1e-1, 1e-1], wu=[1e-2, 3e-2],
          wf=[1e0, 1e1, 1e-1, 1e-1], u_bound=8.0, wrap_index=1)
VC_GAIN, VC_LEVER = 0.1, 0.3
VC_PHYS = (9.81, 0.5, 1.0, 0.2)     # gravity, pole length, cart mass, pole mass


def vectored_cartpole_ode(state, action):
    g, pl, mc, mp = VC_PHYS
    mt = mc + mp
    _, th, xd, thd = state
    u = np.atleast_1d(action)
    fh = u[0] * np.cos(VC_GAIN * u[1])
    fv = u[0] * np.sin(VC_GAIN * u[1])
    s, c = np.sin(th), np.cos(th)
    xdd = (fh + mp * s * (pl * thd ** 2 + g * c)) / (mc + mp * s ** 2)
    thdd = (-fh * c - mp * pl * thd ** 2 * c * s - mt * g * s + VC_LEVER * fv) / (
        pl * mc + pl * mp * s ** 2)
    return np.hstack((xd, thd, xdd, thdd))


def vectored_cartpole(dt, build=True):
    from noc import families
    return families.register_family("vectored_cartpole", vectored_cartpole_ode, dt=dt, build=build,
                                    **VC)


def _param_cost_torch(spec, wrap):
    """constraints / stage / final / total of the parametrised cost (noc.families) in torch"""
    import torch
    from oracle import problems as PR
    goal = torch.tensor(spec["goal"])
    Wx, Wf = torch.diag(torch.tensor(spec["wx"])), torch.diag(torch.tensor(spec["wf"]))
    Wu = torch.diag(torch.tensor(spec["wu"]))
    ub = spec["u_bound"]

    def constraints(state, control):
        return torch.cat((control - ub, -control - ub))

    def err(state):
        return torch.stack([PR.wrap_angle(state[i]) if i == wrap else state[i]
                            for i in range(spec["nx"])]) - goal

    def final_cost(state):
        e = err(state)
        return 0.5 * e @ Wf @ e

    def stage_cost(state, action, bp):
        e = err(state)
        c = 0.5 * e @ Wx @ e + 0.5 * action @ Wu @ action
        return c - bp * torch.sum(torch.log(-constraints(state, action)))

    def total_cost(states, controls, bp):
        ct = torch.func.vmap(stage_cost, in_dims=(0, 0, None))(states[:-1], controls, bp)
        return final_cost(states[-1]) + torch.sum(ct)

    return constraints, stage_cost, final_cost, total_cost


def vectored_cartpole_torch(dt):
    """The same problem restated in torch (oracle/problems.py conventions) for torch.func."""
    import torch
    from oracle import problems as PR

    def ode(state, action):
        g, pl, mc, mp = VC_PHYS
        th, xd, thd = state[1], state[2], state[3]
        fh = action[0] * torch.cos(VC_GAIN * action[1])
        fv = action[0] * torch.sin(VC_GAIN * action[1])
        s, c = torch.sin(th), torch.cos(th)
        xdd = (fh + mp * s * (pl * thd ** 2 + g * c)) / (mc + mp * s ** 2)
        thdd = (-fh * c - mp * pl * thd ** 2 * c * s - (mc + mp) * g * s + VC_LEVER * fv) / (
            pl * mc + pl * mp * s ** 2)
        return torch.stack((xd, thd, xdd, thdd))

    return PR.TorchOCP(PR.euler(ode, dt), *_param_cost_torch(VC, VC["wrap_index"]), 4, 2,
                       "vectored_cartpole")


# ------------------------------------------------------------------------------------------------
# reaction_pendulum (nx=3, nu=2, traced costs): state (angle, angular velocity, motor torque);
# u0 is the motor's torque set-point (first-order lag), u1 a direct thruster whose lever shortens
# with cos(angle), and the motor saturates a little with the thruster on (u0 u1 in its lag).
# Constraints: the two control boxes, the shared supply u0 + u1 <= RP_SUPPLY (so the barrier's
# cuu has an off-diagonal), and the motor torque within +-RP_TORQUE (a state constraint).  The
# stage cost couples the velocity with the SECOND control by a constant (cxu[1, 1]) and the angle
# with it through sin (cxu[0, 1] varies); cxx carries constants (the weights) and a varying quartic.
RP_U0, RP_U1, RP_SUPPLY, RP_TORQUE = 4.0, 3.0, 5.0, 6.0
_RP_WX = np.array([1e0, 1e-1, 1e-2])
_RP_WF = np.array([2e0, 2e-1, 1e-2])
_RP_WU = np.array([1e-2, 4e-2])
_RP_GOAL = np.array([math.pi, 0.0, 0.0])
RP_CROSS_U, RP_CROSS_VEL, RP_CROSS_SIN, RP_QUARTIC = 5e-3, 2e-2, 1e-2, 1e-4


def reaction_pendulum_ode(state, action):
    g, damping, lag = 9.81, 0.1, 0.05
    angle, velocity, torque = state
    u = np.atleast_1d(action)
    return np.hstack((velocity,
                      -g * np.sin(angle) - damping * velocity + torque + 0.5 * u[1] * np.cos(angle),
                      (u[0] - torque) / lag - 0.2 * u[0] * u[1]))


def reaction_pendulum_constraints(state, action):
    u = np.atleast_1d(action)
    return np.hstack((u[0] - RP_U0, -u[0] - RP_U0, u[1] - RP_U1, -u[1] - RP_U1,
                      u[0] + u[1] - RP_SUPPLY, state[2] - RP_TORQUE, -state[2] - RP_TORQUE))


def _rp_err(state):
    return np.hstack((state[0] % (2.0 * np.pi), state[1], state[2])) - _RP_GOAL


def reaction_pendulum_final_cost(state):
    e = _rp_err(state)
    return 0.5 * e @ np.diag(_RP_WF) @ e


def reaction_pendulum_stage_cost(state, action, bp):
    e = _rp_err(state)
    u = np.atleast_1d(action)
    c = 0.5 * e @ np.diag(_RP_WX) @ e + 0.5 * u @ np.diag(_RP_WU) @ u + RP_CROSS_U * u[0] * u[1]
    c = c + RP_CROSS_VEL * state[1] * u[1] + RP_CROSS_SIN * np.sin(state[0]) * u[1]
    c = c + RP_QUARTIC * state[1] ** 4
    return c - bp * np.sum(np.log(-reaction_pendulum_constraints(state, action)))


def reaction_pendulum(dt, build=True):
    from noc import families
    return families.register_family("reaction_pendulum", reaction_pendulum_ode, nx=3, nu=2, dt=dt,
                                    stage_cost=reaction_pendulum_stage_cost,
                                    final_cost=reaction_pendulum_final_cost,
                                    constraints=reaction_pendulum_constraints, build=build)


def reaction_pendulum_torch(dt):
    """The same problem restated in torch (oracle/problems.py conventions) for torch.func."""
    import torch
    from oracle import problems as PR
    goal = torch.tensor(_RP_GOAL)
    Wx, Wf = torch.diag(torch.tensor(_RP_WX)), torch.diag(torch.tensor(_RP_WF))
    Wu = torch.diag(torch.tensor(_RP_WU))

    def constraints(state, control):
        return torch.stack((control[0] - RP_U0, -control[0] - RP_U0, control[1] - RP_U1,
                            -control[1] - RP_U1, control[0] + control[1] - RP_SUPPLY,
                            state[2] - RP_TORQUE, -state[2] - RP_TORQUE))

    def err(state):
        return torch.stack((PR.wrap_angle(state[0]), state[1], state[2])) - goal

    def final_cost(state):
        e = err(state)
        return 0.5 * e @ Wf @ e

    def stage_cost(state, action, bp):
        e = err(state)
        c = 0.5 * e @ Wx @ e + 0.5 * action @ Wu @ action + RP_CROSS_U * action[0] * action[1]
        c = c + RP_CROSS_VEL * state[1] * action[1] + RP_CROSS_SIN * torch.sin(state[0]) * action[1]
        c = c + RP_QUARTIC * state[1] ** 4
        return c - bp * torch.sum(torch.log(-constraints(state, action)))

    def total_cost(states, controls, bp):
        ct = torch.func.vmap(stage_cost, in_dims=(0, 0, None))(states[:-1], controls, bp)
        return final_cost(states[-1]) + torch.sum(ct)

    def ode(state, action):
        g, damping, lag = 9.81, 0.1, 0.05
        return torch.stack((state[1],
                            -g * torch.sin(state[0]) - damping * state[1] + state[2]
                            + 0.5 * action[1] * torch.cos(state[0]),
                            (action[0] - state[2]) / lag - 0.2 * action[0] * action[1]))

    return PR.TorchOCP(PR.euler(ode, dt), constraints, stage_cost, final_cost, total_cost, 3, 2,
                       "reaction_pendulum")


# ------------------------------------------------------------------------------------------------
# triple_drive_pendulum (nx=2, nu=3, parametrised cost): more controls than states.  A pendulum
# with three actuators of different gains: a direct torque, one saturating through tanh (fuu has a
# non-zero diagonal) and a thruster whose lever is cos(angle) (fxu is non-zero).  R is 3 x 3.
TD = dict(nx=2, nu=3, goal=[math.pi, 0.0], wx=[1e0, 1e-1], wu=[1e-3, 4e-3, 9e-3], wf=[1e0, 1e-1],
          u_bound=3.0, wrap_index=0)
TD_GAINS = (1.0, 2.5, 0.6)


def triple_drive_pendulum_ode(state, action):
    g, length, damping = 9.81, 1.0, 1e-2
    angle, velocity = state
    u = np.atleast_1d(action)
    torque = TD_GAINS[0] * u[0] + TD_GAINS[1] * np.tanh(u[1]) + TD_GAINS[2] * u[2] * np.cos(angle)
    return np.hstack((velocity, -g / length * np.sin(angle) - damping * velocity + torque))


def triple_drive_pendulum(dt, build=True):
    from noc import families
    return families.register_family("triple_drive_pendulum", triple_drive_pendulum_ode, dt=dt,
                                    build=build, **TD)


def triple_drive_pendulum_torch(dt):
    """The same problem restated in torch (oracle/problems.py conventions) for torch.func."""
    import torch
    from oracle import problems as PR

    def ode(state, action):
        g, length, damping = 9.81, 1.0, 1e-2
        torque = (TD_GAINS[0] * action[0] + TD_GAINS[1] * torch.tanh(action[1])
                  + TD_GAINS[2] * action[2] * torch.cos(state[0]))
        return torch.stack((state[1], -g / length * torch.sin(state[0]) - damping * state[1] + torque))

    return PR.TorchOCP(PR.euler(ode, dt), *_param_cost_torch(TD, TD["wrap_index"]), 2, 3,
                       "triple_drive_pendulum")


MULTI_CONTROL = {"vectored_cartpole": (vectored_cartpole, vectored_cartpole_torch),
                 "reaction_pendulum": (reaction_pendulum, reaction_pendulum_torch),
                 "triple_drive_pendulum": (triple_drive_pendulum, triple_drive_pendulum_torch)}
MULTI_CONTROL_DT = 1.0 / 24


def build_all(verbose=False):
    """Register (and build once) every test family; returns their OCPs."""
    return [actuated_pendulum(1.0 / 50), cartpole_track_limit(1.0 / 50)] + \
        [reg(MULTI_CONTROL_DT) for reg, _ in MULTI_CONTROL.values()]
