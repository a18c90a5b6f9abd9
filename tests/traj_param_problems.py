"""Oracle problems with explicit cost parameters (test infrastructure): the pendulum and cart-pole
of oracle/problems.py with goal, weights and control bound as arguments, as torch callables for
oracle.noc_oracle.NumpyProblem (torch.func autodiff), so that a heterogeneous batch's row b can be
checked against an oracle solve of its own problem, independently of the project's kernels.
The dynamics are the oracle's own (examples/pendulum_runtime.py:59-72, cartpole_runtime.py:54-81);
the costs restate PR:30-56 / CR:27-51 with the constants replaced by the arguments."""
import numpy as np
import torch
from torch.func import vmap

from oracle import noc_oracle as O
from oracle import problems as PR


def _param_ocp(base: PR.TorchOCP, wrap_index: int, goal, wx, wu, wf, u_bound) -> PR.TorchOCP:
    goal_t = torch.as_tensor(np.asarray(goal, dtype=np.float64))
    Wx = torch.diag(torch.as_tensor(np.asarray(wx, dtype=np.float64)))
    Wu = torch.diag(torch.as_tensor(np.asarray(wu, dtype=np.float64)))
    Wf = torch.diag(torch.as_tensor(np.asarray(wf, dtype=np.float64)))
    ub = float(u_bound)

    def constraints(state, control):
        return torch.cat((control - ub, -control - ub))

    def _err(state):
        parts = [PR.wrap_angle(state[i]) if i == wrap_index else state[i] for i in range(base.nx)]
        return torch.stack(parts) - goal_t

    def final_cost(state):
        e = _err(state)
        return 0.5 * e @ Wf @ e

    def stage_cost(state, action, bp):
        e = _err(state)
        c = 0.5 * e @ Wx @ e + 0.5 * action @ Wu @ action
        return c - bp * torch.sum(torch.log(-constraints(state, action)))

    def total_cost(states, controls, bp):
        ct = vmap(stage_cost, in_dims=(0, 0, None))(states[:-1], controls, bp)
        return final_cost(states[-1]) + torch.sum(ct)

    return PR.TorchOCP(base.dynamics, constraints, stage_cost, final_cost, total_cost, base.nx,
                       base.nu, base.name + "_params")


def pendulum_problem(dt, goal, wx, wu, wf, u_bound) -> O.NumpyProblem:
    return O.NumpyProblem(_param_ocp(PR.pendulum_ocp(dt), 0, goal, wx, wu, wf, u_bound))


def cartpole_problem(dt, goal, wx, wu, wf, u_bound) -> O.NumpyProblem:
    return O.NumpyProblem(_param_ocp(PR.cartpole_ocp(dt), 1, goal, wx, wu, wf, u_bound))
