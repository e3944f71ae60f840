"""ctypes binding of libso100sim.so (C ABI: include/so100_sim.h).

PyTorch is plumbing here: it owns device memory and streams; every tensor crosses the boundary as a raw
device pointer (`tensor.data_ptr()`) plus the current HIP stream handle.  There is NO CPU fallback: if the
shared object is missing or no HIP device is usable, loading / `So100Sim()` raises.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import torch  # imported BEFORE the .so so that both bind to the same libamdhip64 (see csrc/Makefile)

from . import constants as K

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SO100_LIB", os.path.join(_HERE, "libso100sim.so"))   # SO100_LIB: A/B builds of the same ABI (tools/)

ENV01, ENV02, ENV03, ENV04, ENV05, ENV06 = 1, 2, 3, 4, 5, 6
F_FRICTIONLOSS, F_LIMITS, F_FLOOR, F_CUBE_PINNED, F_PADS_FLOOR, F_PADS_CUBE, F_LINKS_FLOOR, F_LINKS_CUBE = 1, 2, 4, 8, 16, 32, 64, 128
F_REFERENCE = F_FRICTIONLOSS | F_LIMITS | F_FLOOR | F_PADS_FLOOR     # what the reference scene simulates (minus its mesh geoms)
F_NOPADS = F_FRICTIONLOSS | F_LIMITS | F_FLOOR                         # round-1 "reference": no arm contact at all
F_CONTACT5 = F_REFERENCE | F_PADS_CUBE                                  # BASELINE.json configs[4]: finger pads vs cube, coupled solve
F_REFERENCE_LINKS = F_REFERENCE | F_LINKS_FLOOR                         # + capsule proxies of the arm's collision meshes vs the floor (a documented stand-in)
F_REFERENCE_PROXIES = F_REFERENCE_LINKS | F_LINKS_CUBE                  # + Rotation_Pitch / Upper_Arm capsules vs the cube (needs a dynamic cube)
B_BAD_STATE = 128            # bit of the `bits` state row latched when a non-finite state ended an episode (csrc/so100_task.hpp)
NINJECT = 16
ABI_VERSION = 3              # include/so100_sim.h: SO100_ABI_VERSION


class So100Error(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [("env_kind", C.c_int32), ("num_envs", C.c_int32), ("device", C.c_int32), ("flags", C.c_uint32),
                ("solver_iters", C.c_int32), ("contact_iters", C.c_int32), ("frame_skip", C.c_int32),
                ("max_episode_steps", C.c_int32), ("seed", C.c_uint64), ("env_id_offset", C.c_uint32),
                ("envs_per_workgroup", C.c_uint32)]


class StepIO(C.Structure):
    _fields_ = [("act_dev", C.c_void_p), ("obs_dev", C.c_void_p), ("rew_dev", C.c_void_p), ("done_dev", C.c_void_p),
                ("trunc_dev", C.c_void_p), ("terminal_obs_dev", C.c_void_p), ("ep_return_dev", C.c_void_p),
                ("ep_length_dev", C.c_void_p), ("inject_dev", C.c_void_p), ("rollout_row_dev", C.c_void_p)]


POLICY_TENSORS = ["pi_w0", "pi_b0", "pi_w1", "pi_b1", "mu_w", "mu_b", "log_std", "vf_w0", "vf_b0", "vf_w1", "vf_b1", "v_w", "v_b"]
# the SB3 ActorCriticPolicy state_dict entry behind each pointer
SB3_STATE_DICT_KEYS = {"pi_w0": "mlp_extractor.policy_net.0.weight", "pi_b0": "mlp_extractor.policy_net.0.bias",
                       "pi_w1": "mlp_extractor.policy_net.2.weight", "pi_b1": "mlp_extractor.policy_net.2.bias",
                       "mu_w": "action_net.weight", "mu_b": "action_net.bias", "log_std": "log_std",
                       "vf_w0": "mlp_extractor.value_net.0.weight", "vf_b0": "mlp_extractor.value_net.0.bias",
                       "vf_w1": "mlp_extractor.value_net.2.weight", "vf_b1": "mlp_extractor.value_net.2.bias",
                       "v_w": "value_net.weight", "v_b": "value_net.bias"}


class PolicyWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in POLICY_TENSORS]


def policy_tensor_shapes(obs_dim):
    """{name: PyTorch shape} of the policy's tensors (csrc/so100_policy_tensors.h: nn.Linear layout, 2 x 64 towers, 6 actions)"""
    tower = lambda p: {p + "_w0": (64, obs_dim), p + "_b0": (64,), p + "_w1": (64, 64), p + "_b1": (64,)}
    shapes = {**tower("pi"), "mu_w": (6, 64), "mu_b": (6,), "log_std": (6,), **tower("vf"), "v_w": (1, 64), "v_b": (1,)}
    assert list(shapes) == POLICY_TENSORS
    return shapes


class RolloutIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("rollout_dev", "obs_dev", "rew_dev", "done_dev", "trunc_dev", "terminal_obs_dev",
                                          "ep_return_dev", "ep_length_dev", "terminal_obs_chunk_dev")]


class RenderIO(C.Structure):
    _fields_ = [("camera", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("env_begin", C.c_int32), ("env_count", C.c_int32),
                ("geom_mask", C.c_uint32), ("free_cam", C.c_void_p), ("rgb_dev", C.c_void_p), ("depth_dev", C.c_void_p), ("seg_dev", C.c_void_p)]


CAM_END, CAM_SCENE = 0, 1                       # include/so100_sim.h: SO100_CAM_*
CAMERAS = {"end": CAM_END, "scene": CAM_SCENE}
G_FLOOR, G_CUBE, G_LINKS, G_PADS = 1, 2, 4, 8   # SO100_GEOM_*: geometry bits of so100_render
GEOM_NAMES = {"floor": G_FLOOR, "cube": G_CUBE, "links": G_LINKS, "pads": G_PADS}


class PolicyIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("obs_dev", "noise_dev", "act_env_dev", "act_raw_dev", "value_dev", "logp_dev", "rollout_row_dev")]


EXPORTS = ["so100_abi_version", "so100_obs_dim", "so100_num_state_fields", "so100_state_field_index", "so100_state_field_name", "so100_create",
           "so100_envs_per_workgroup", "so100_destroy", "so100_reset", "so100_step", "so100_get_state", "so100_set_state", "so100_get_field",
           "so100_set_field", "so100_last_error", "so100_policy_forward", "so100_rollout", "so100_render"]


# ---- include/so100_learn.h: the on-device PPO learner (additive: EXPORTS above is the list of so100_sim.h alone) -----------------------
class LearnerConfig(C.Structure):
    _fields_ = [("obs_dim", C.c_int32), ("device", C.c_int32), ("max_minibatch", C.c_int32), ("gamma", C.c_float), ("gae_lambda", C.c_float),
                ("clip_range", C.c_float), ("vf_coef", C.c_float), ("max_grad_norm", C.c_float), ("lr", C.c_double), ("beta1", C.c_double),
                ("beta2", C.c_double), ("adam_eps", C.c_double)]


class AdvantagesIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("rollout_dev", "terminal_obs_chunk_dev", "last_obs_dev", "params_dev", "adv_dev", "ret_dev", "adv_stats_dev")]


class MinibatchIO(C.Structure):
    _fields_ = [("rollout_dev", C.c_void_p), ("num_samples", C.c_int64), ("idx_dev", C.c_void_p), ("mb", C.c_int32), ("adam_step", C.c_int32),
                ("adv_dev", C.c_void_p), ("ret_dev", C.c_void_p), ("adv_stats_dev", C.c_void_p), ("params_dev", C.c_void_p), ("adam_m_dev", C.c_void_p),
                ("adam_v_dev", C.c_void_p), ("stats_dev", C.c_void_p), ("grads_dev", C.c_void_p)]


class PpoTerms(C.Structure):
    _fields_ = [("ent_coef", C.c_float), ("clip_range_vf", C.c_float), ("normalize_advantage", C.c_int32), ("target_kl", C.c_float), ("lr", C.c_double)]


UPDATE_OUT = 15              # include/so100_learn.h: SO100_UPDATE_OUT


class UpdateIO(C.Structure):
    _fields_ = [("rollout_dev", C.c_void_p), ("terminal_obs_chunk_dev", C.c_void_p), ("last_obs_dev", C.c_void_p), ("T", C.c_int32), ("N", C.c_int32),
                ("params_dev", C.c_void_p), ("adam_m_dev", C.c_void_p), ("adam_v_dev", C.c_void_p), ("adv_dev", C.c_void_p), ("ret_dev", C.c_void_p),
                ("adv_stats_dev", C.c_void_p), ("perm_dev", C.c_void_p), ("epochs", C.c_int32), ("mb", C.c_int32), ("adam_step0", C.c_int32),
                ("shuffle_epoch0", C.c_uint32), ("shuffle_seed", C.c_uint64), ("terms", C.POINTER(PpoTerms)), ("update_state_dev", C.c_void_p),
                ("out_dev", C.c_void_p)]


class RewardNormIO(C.Structure):
    _fields_ = [("rollout_dev", C.c_void_p), ("state_dev", C.c_void_p), ("reward_dev", C.c_void_p), ("workspace_dev", C.c_void_p),
                ("workspace_bytes", C.c_int64), ("clip_reward", C.c_double), ("epsilon", C.c_double)]


class ObsNormIO(C.Structure):
    _fields_ = [("rollout_dev", C.c_void_p), ("state_dev", C.c_void_p), ("workspace_dev", C.c_void_p), ("workspace_bytes", C.c_int64)]


OBS_NORM_EPSILON = 1e-8                                # SB3 VecNormalize's epsilon
REWARD_NORM_EPSILON, REWARD_NORM_CLIP = 1e-8, 10.0     # SB3 VecNormalize's epsilon and clip_reward
REWARD_NORM_INIT = (0.0, 1.0, 1e-4)                    # mean, var, count of a fresh RunningMeanStd (so100_learner_reward_norm_init)

LEARN_EXPORTS = ["so100_learner_num_params", "so100_learner_param_offset", "so100_learner_param_size", "so100_learner_create", "so100_learner_destroy",
                 "so100_learner_advantages", "so100_learner_minibatch_step", "so100_learner_minibatch_step_ex", "so100_learner_explained_variance",
                 "so100_learner_shuffle", "so100_learner_update", "so100_learner_reward_norm_workspace", "so100_learner_reward_norm_init",
                 "so100_learner_normalize_rewards", "so100_learner_advantages_r", "so100_learner_update_r", "so100_learner_obs_norm_init",
                 "so100_learner_obs_norm_workspace", "so100_learner_obs_norm_update", "so100_learner_obs_norm_fold", "so100_learner_set_obs_norm"]
LEARNER_STATS = ["policy_loss", "value_loss", "clip_fraction", "grad_norm"]          # stats_dev[4] of so100_learner_minibatch_step
LEARNER_DIAG = LEARNER_STATS + ["approx_kl", "entropy_loss", "loss", "value_clip_fraction"]       # diag_dev[8] of so100_learner_minibatch_step_ex
NORMALIZE_ADVANTAGE = {"batch": 0, "minibatch": 1}                                   # so100_ppo_terms.normalize_advantage


# ---- include/so100_query.h: model queries (additive like the learner: EXPORTS above is the list of so100_sim.h alone) -------------------------
class KinematicsIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("q_dev", "xpos_dev", "xmat_dev", "ee_dev", "cam_pos_dev", "cam_mat_dev")]


class JacobianIO(C.Structure):
    _fields_ = [("q_dev", C.c_void_p), ("link", C.c_int32), ("offset", C.c_void_p), ("jacp_dev", C.c_void_p), ("jacr_dev", C.c_void_p)]


class DynamicsIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("q_dev", "v_dev", "qacc_dev", "M_dev", "bias_dev", "tau_dev")]


class IkIO(C.Structure):
    _fields_ = [("target_dev", C.c_void_p), ("q0_dev", C.c_void_p), ("link", C.c_int32), ("offset", C.c_void_p), ("iters", C.c_int32),
                ("damping", C.c_float), ("tol", C.c_float), ("max_step", C.c_float), ("q_dev", C.c_void_p), ("residual_dev", C.c_void_p),
                ("iterations_dev", C.c_void_p), ("converged_dev", C.c_void_p)]


class ForwardIO(C.Structure):
    _fields_ = [("qpos_dev", C.c_void_p), ("qvel_dev", C.c_void_p), ("ctrl_dev", C.c_void_p), ("flags", C.c_uint32), ("solver_iters", C.c_int32),
                ("contact_iters", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("qacc_dev", "qfrc_constraint_dev", "ncon_dev", "dropped_dev", "con_kind_dev", "con_feat_dev", "con_pos_dev",
                                          "con_frame_dev", "con_dist_dev", "con_force_dev", "pad_force_dev", "residual_dev")]


class TrajectoryIO(C.Structure):
    _fields_ = [("qpos_dev", C.c_void_p), ("qvel_dev", C.c_void_p), ("ctrl_dev", C.c_void_p), ("mode", C.c_int32), ("T", C.c_int32), ("nsub", C.c_int32),
                ("flags", C.c_uint32), ("solver_iters", C.c_int32), ("contact_iters", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("qpos_traj_dev", "qvel_traj_dev", "ee_traj_dev", "qpos_final_dev", "qvel_final_dev", "ncon_dev", "dropped_dev",
                                          "sig_dev", "residual_dev", "bad_step_dev")]


class DerivativesIO(C.Structure):
    _fields_ = [("qpos_dev", C.c_void_p), ("qvel_dev", C.c_void_p), ("ctrl_dev", C.c_void_p), ("mode", C.c_int32), ("nsub", C.c_int32),
                ("flags", C.c_uint32), ("solver_iters", C.c_int32), ("contact_iters", C.c_int32), ("eps", C.c_float)] + \
               [(n, C.c_void_p) for n in ("A_dev", "B_dev", "qpos_next_dev", "qvel_next_dev", "bad_dev")]


class LqrIO(C.Structure):
    _fields_ = [("nx", C.c_int32), ("T", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("A_dev", "B_dev", "lx_dev", "lxx_dev", "lu_dev", "luu_dev", "lux_dev", "u_dev", "dx0_dev")] + \
               [(n, C.c_float) for n in ("reg", "alpha", "u_lo", "u_hi")] + \
               [(n, C.c_void_p) for n in ("k_dev", "K_dev", "Vx0_dev", "Vxx0_dev", "dV_dev", "du_dev", "dx_dev", "bad_dev")]


class LqrRegIO(C.Structure):
    _fields_ = [("base", LqrIO), ("reg_dev", C.c_void_p), ("reg_min", C.c_float), ("reg_max", C.c_float), ("reg_up", C.c_float), ("tries", C.c_int32),
                ("reg_used_dev", C.c_void_p), ("tries_dev", C.c_void_p)]


class RegScheduleIO(C.Structure):
    _fields_ = [("reg_used_dev", C.c_void_p), ("best_dev", C.c_void_p), ("keep", C.c_int32), ("reg_min", C.c_float), ("reg_max", C.c_float),
                ("reg_up", C.c_float), ("reg_down", C.c_float), ("reg_dev", C.c_void_p), ("improved_dev", C.c_void_p)]


class ClosedLoopIO(C.Structure):
    _fields_ = [("qpos_dev", C.c_void_p), ("qvel_dev", C.c_void_p), ("u_dev", C.c_void_p), ("mode", C.c_int32), ("T", C.c_int32), ("nsub", C.c_int32),
                ("flags", C.c_uint32), ("solver_iters", C.c_int32), ("contact_iters", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("qpos_ref_dev", "qvel_ref_dev", "qpos_ref0_dev", "qvel_ref0_dev")] + \
               [("nx", C.c_int32), ("k_dev", C.c_void_p), ("K_dev", C.c_void_p), ("L", C.c_int32), ("alpha", C.c_void_p), ("clamp", C.c_int32),
                ("u_lo", C.c_float), ("u_hi", C.c_float)] + \
               [(n, C.c_void_p) for n in ("u_traj_dev", "qpos_traj_dev", "qvel_traj_dev", "ee_traj_dev", "qpos_final_dev", "qvel_final_dev", "ncon_dev",
                                          "dropped_dev", "sig_dev", "residual_dev", "bad_step_dev")]


class CostDef(C.Structure):
    _fields_ = [("link", C.c_int32), ("offset", C.c_void_p), ("target_mode", C.c_int32), ("w_point", C.c_float), ("w_q", C.c_float*6), ("q_nom", C.c_float*6),
                ("w_v", C.c_float*6), ("w_u", C.c_float*6), ("w_terminal", C.c_float)]


class CostTermsIO(C.Structure):
    _fields_ = [("cost", C.POINTER(CostDef)), ("target_dev", C.c_void_p), ("nx", C.c_int32), ("T", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("qpos_traj_dev", "qvel_traj_dev", "u_dev", "lx_dev", "lxx_dev", "lu_dev", "luu_dev")]


class CostSelectIO(C.Structure):
    _fields_ = [("cost", C.POINTER(CostDef)), ("target_dev", C.c_void_p), ("T", C.c_int32), ("L", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("qpos_traj_dev", "qvel_traj_dev", "u_traj_dev", "bad_step_dev", "u_fallback_dev", "cost_dev", "best_dev", "best_cost_dev",
                                          "u_best_dev")]


class PlanSampleIO(C.Structure):
    _fields_ = [("plan_dev", C.c_void_p), ("sigma", C.c_float*6), ("u_lo", C.c_float), ("u_hi", C.c_float), ("K", C.c_int32), ("T", C.c_int32),
                ("seed", C.c_uint64), ("draw", C.c_uint32), ("id_offset", C.c_uint32)] + \
               [(n, C.c_void_p) for n in ("qpos_dev", "qvel_dev", "ctrl_dev", "qpos_rep_dev", "qvel_rep_dev")]


class CostBlendIO(C.Structure):
    _fields_ = [("cost", C.POINTER(CostDef)), ("target_dev", C.c_void_p), ("T", C.c_int32), ("K", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("qpos_traj_dev", "qvel_traj_dev", "u_traj_dev", "bad_step_dev", "u_fallback_dev")] + \
               [("temperature", C.c_float), ("shift", C.c_int32), ("tail", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("cost_dev", "best_dev", "best_cost_dev", "weight_dev", "ess_dev", "u_plan_dev", "u_first_dev")]


class PlanSampleTvIO(C.Structure):
    _fields_ = [("plan_dev", C.c_void_p), ("sigma_dev", C.c_void_p), ("u_lo", C.c_float), ("u_hi", C.c_float), ("K", C.c_int32), ("T", C.c_int32),
                ("seed", C.c_uint64), ("draw", C.c_uint32), ("id_offset", C.c_uint32)] + \
               [(n, C.c_void_p) for n in ("qpos_dev", "qvel_dev", "ctrl_dev", "qpos_rep_dev", "qvel_rep_dev")]


class CostRefitIO(C.Structure):
    _fields_ = [("cost", C.POINTER(CostDef)), ("target_dev", C.c_void_p), ("T", C.c_int32), ("K", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("qpos_traj_dev", "qvel_traj_dev", "u_traj_dev", "bad_step_dev", "u_fallback_dev")] + \
               [("E", C.c_int32), ("alpha", C.c_float), ("plan_dev", C.c_void_p), ("sigma_dev", C.c_void_p), ("sigma_min", C.c_float*6), ("sigma_max", C.c_float*6),
                ("sigma_init", C.c_float*6), ("shift", C.c_int32), ("tail", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("cost_dev", "best_dev", "best_cost_dev", "elite_dev", "n_elite_dev", "threshold_dev", "mean_dev", "sigma_out_dev",
                                          "u_first_dev")]


QUERY_EXPORTS = ["so100_query_kinematics", "so100_query_jacobian", "so100_query_dynamics", "so100_query_ik", "so100_query_forward",
                 "so100_query_trajectory", "so100_query_derivatives", "so100_query_lqr", "so100_query_closed_loop", "so100_query_cost_terms",
                 "so100_query_cost_select", "so100_query_plan_sample", "so100_query_cost_blend", "so100_query_plan_sample_tv", "so100_query_cost_refit",
                 "so100_query_lqr_reg", "so100_query_reg_schedule"]
QUERY_IO = {"so100_query_kinematics": KinematicsIO, "so100_query_jacobian": JacobianIO, "so100_query_dynamics": DynamicsIO, "so100_query_ik": IkIO,
            "so100_query_forward": ForwardIO, "so100_query_trajectory": TrajectoryIO, "so100_query_derivatives": DerivativesIO, "so100_query_lqr": LqrIO,
            "so100_query_closed_loop": ClosedLoopIO, "so100_query_cost_terms": CostTermsIO, "so100_query_cost_select": CostSelectIO,
            "so100_query_plan_sample": PlanSampleIO, "so100_query_cost_blend": CostBlendIO, "so100_query_plan_sample_tv": PlanSampleTvIO,
            "so100_query_cost_refit": CostRefitIO, "so100_query_lqr_reg": LqrRegIO, "so100_query_reg_schedule": RegScheduleIO}
MPPI_MAX_K = 4096                                              # SO100_MPPI_MAX_K
BLEND_TAILS = {"zero": 0, "hold": 1}                           # SO100_BLEND_TAIL_*
COST_TARGETS = {"fixed": 0, "traj": 1, "cube": 2}               # SO100_COST_TARGET_*
DERIV_NX, DERIV_NU, DERIV_EPS = 24, 6, 2.0**-6                 # SO100_DERIV_*
LQR_NU, LQR_MAX_T, LQR_REG_MAX_TRIES = 6, 4096, 16             # SO100_LQR_*
CL_MAX_L = 16                                                  # SO100_CL_MAX_L
TRAJ_MODES = {"targets": 0, "actions": 1}                      # SO100_TRAJ_TARGETS / SO100_TRAJ_ACTIONS
TRAJ_MAX_T, TRAJ_MAX_NSUB, TRAJ_MAX_SUBSTEPS = 4096, 1024, 65536    # SO100_TRAJ_MAX_*
EE_LINK = 4                                                    # SO100_EE_LINK: the reference's end-effector point sits on Fixed_Jaw
IK_ITERS, IK_DAMPING, IK_TOL, IK_MAX_STEP = 64, 0.02, 1e-4, 0.3     # SO100_IK_*
FWD_MAXCON, FWD_SOLVER_ITERS, FWD_CONTACT_ITERS = 20, 64, 64        # SO100_FWD_*


def build(verbose=False):
    """Compile libso100sim.so for gfx950 (hipcc cross-compiles without a GPU)."""
    out = subprocess.run(["make", "-j7", "-C", os.path.join(_HERE, "csrc")], capture_output=True, text=True)
    if out.returncode != 0:
        raise So100Error("building libso100sim.so failed:\n" + out.stdout[-4000:] + out.stderr[-4000:])
    if verbose:
        print(out.stdout[-3000:])
    return LIB_PATH


_lib = None


def load():
    """dlopen the shared object (built in-tree; never falls back to anything else)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise So100Error(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        L.so100_last_error.restype = C.c_char_p
        L.so100_state_field_index.argtypes = [C.c_char_p]
        L.so100_state_field_name.argtypes = [C.c_int32]; L.so100_state_field_name.restype = C.c_char_p
        L.so100_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
        L.so100_envs_per_workgroup.argtypes = [C.c_void_p]
        L.so100_destroy.argtypes = [C.c_void_p]
        L.so100_destroy.restype = None
        L.so100_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.so100_step.argtypes = [C.c_void_p, C.POINTER(StepIO), C.c_void_p]
        L.so100_policy_forward.argtypes = [C.c_void_p, C.POINTER(PolicyWeights), C.POINTER(PolicyIO), C.c_uint32, C.c_void_p]
        L.so100_rollout.argtypes = [C.c_void_p, C.POINTER(PolicyWeights), C.POINTER(RolloutIO), C.c_int32, C.c_uint32, C.c_void_p]
        L.so100_get_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.so100_set_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.so100_get_field.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.so100_set_field.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.so100_render.argtypes = [C.c_void_p, C.POINTER(RenderIO), C.c_void_p]
        L.so100_learner_num_params.argtypes = [C.c_int32]
        L.so100_learner_param_offset.argtypes = [C.c_int32, C.c_char_p]
        L.so100_learner_param_size.argtypes = [C.c_int32, C.c_char_p]
        L.so100_learner_create.argtypes = [C.POINTER(LearnerConfig), C.POINTER(C.c_void_p)]
        L.so100_learner_destroy.argtypes = [C.c_void_p]
        L.so100_learner_destroy.restype = None
        L.so100_learner_advantages.argtypes = [C.c_void_p, C.POINTER(AdvantagesIO), C.c_int32, C.c_int32, C.c_void_p]
        L.so100_learner_minibatch_step.argtypes = [C.c_void_p, C.POINTER(MinibatchIO), C.c_void_p]
        L.so100_learner_minibatch_step_ex.argtypes = [C.c_void_p, C.POINTER(MinibatchIO), C.POINTER(PpoTerms), C.c_void_p, C.c_void_p, C.c_void_p]
        L.so100_learner_explained_variance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.so100_learner_shuffle.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int64, C.c_void_p, C.c_void_p]
        L.so100_learner_update.argtypes = [C.c_void_p, C.POINTER(UpdateIO), C.c_void_p]
        L.so100_learner_reward_norm_workspace.argtypes = [C.c_int32, C.c_int32]; L.so100_learner_reward_norm_workspace.restype = C.c_int64
        L.so100_learner_reward_norm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.so100_learner_normalize_rewards.argtypes = [C.c_void_p, C.POINTER(RewardNormIO), C.c_int32, C.c_int32, C.c_void_p]
        L.so100_learner_advantages_r.argtypes = [C.c_void_p, C.POINTER(AdvantagesIO), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        L.so100_learner_update_r.argtypes = [C.c_void_p, C.POINTER(UpdateIO), C.POINTER(RewardNormIO), C.c_void_p]
        L.so100_learner_obs_norm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.so100_learner_obs_norm_workspace.argtypes = [C.c_int32, C.c_int32]; L.so100_learner_obs_norm_workspace.restype = C.c_int64
        L.so100_learner_obs_norm_update.argtypes = [C.c_void_p, C.POINTER(ObsNormIO), C.c_int32, C.c_int32, C.c_void_p]
        L.so100_learner_obs_norm_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.so100_learner_set_obs_norm.argtypes = [C.c_void_p, C.c_void_p]
        for fn, io in QUERY_IO.items():
            getattr(L, fn).argtypes = [C.c_void_p, C.POINTER(io), C.c_int32, C.c_void_p]
        if L.so100_abi_version() != ABI_VERSION:
            raise So100Error("libso100sim.so ABI version mismatch")
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise So100Error(f"{what} failed ({rc}): {load().so100_last_error().decode()}")


def _hptr(t, dtype, shape):
    """pointer of a PINNED host tensor (hipHostMalloc memory is mapped into the GPU's address space at the same address)"""
    if t is None:
        return None
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device.type != "cpu" or not t.is_pinned():
        raise So100Error(f"bad tensor: want {dtype} {tuple(shape)} contiguous in pinned host memory, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t.data_ptr()


def _ptr(t, dtype, shape, device):
    if t is None:
        return None
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != device:
        raise So100Error(f"bad tensor: want {dtype} {tuple(shape)} contiguous on {device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t.data_ptr()


def _optr(t):
    """pointer of a tensor the caller has already laid out, or None (a null pointer: the argument is optional)"""
    return None if t is None else t.data_ptr()


def _resolve_device(device, what, hip_only=False):
    """the torch.device (with its ordinal) a handle lives on: `device`, or torch's current HIP device where it names none"""
    if not torch.cuda.is_available():
        raise So100Error(f"no HIP device visible to PyTorch: {what} has no CPU fallback")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if hip_only and device.type != "cuda":
        raise So100Error(f"{what} runs on a HIP device, not on {device}")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class _Handle:
    """What the two handle classes share: the library, the device, the configuration struct, the native handle made by `create(cfg, &h)`
    and freed by `destroy(h)` on close() or collection, and torch's current stream on the device."""
    _create = _destroy = None        # export names

    def _open(self, device, cfg):
        self.L = load()
        self.device, self.cfg = device, cfg
        h = C.c_void_p()
        _check(getattr(self.L, self._create)(C.byref(cfg), C.byref(h)), self._create)
        self.h = h

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def close(self):
        if getattr(self, "h", None):
            getattr(self.L, self._destroy)(self.h)
            self.h = None

    __del__ = close


def _refreshed(name):
    """a device tensor of So100Sim that step_host() may have left stale: brought up to date on its first read"""
    return property(lambda self: (self._refresh(), getattr(self, name))[1])


class So100Sim(_Handle):
    """One batched simulator handle on one GPU (one per process per device)."""
    _create, _destroy = "so100_create", "so100_destroy"

    def __init__(self, env_kind, num_envs, device=None, flags=F_REFERENCE, solver_iters=2, contact_iters=20,
                 frame_skip=16, max_episode_steps=None, seed=0, env_id_offset=0, envs_per_workgroup=0):
        device = _resolve_device(device, "so100")
        if max_episode_steps is None:
            max_episode_steps = 4000 if env_kind == ENV01 else 6000       # ref: so100_mujoco_rl/__init__.py:5-45
        self._open(device, Config(env_kind, num_envs, device.index, flags, solver_iters, contact_iters, frame_skip,
                                  max_episode_steps, seed, env_id_offset, envs_per_workgroup))
        self.envs_per_workgroup = self.L.so100_envs_per_workgroup(self.h)     # in use (chosen by the library when 0 was passed): part of a checkpoint's configuration
        self.n = num_envs
        self.kind = env_kind
        self.obs_dim = self.L.so100_obs_dim(env_kind)
        kw = dict(device=self.device)
        # the handle's device-side outputs (read through the properties below: a step_host() leaves them stale until then)
        self._obs = torch.zeros(num_envs, self.obs_dim, dtype=torch.float32, **kw)
        self._rew = torch.zeros(num_envs, dtype=torch.float32, **kw)
        self._done = torch.zeros(num_envs, dtype=torch.uint8, **kw)
        self._trunc = torch.zeros(num_envs, dtype=torch.uint8, **kw)
        self._terminal_obs = torch.zeros(num_envs, self.obs_dim, dtype=torch.float32, **kw)
        self._ep_return = torch.zeros(num_envs, dtype=torch.float32, **kw)
        self._ep_length = torch.zeros(num_envs, dtype=torch.int32, **kw)
        self._host_out = None        # pinned host buffers of the last step_host() while they are newer than the device tensors
        self._io = StepIO()

    # obs / rew / done / trunc / terminal_obs / ep_return / ep_length: device tensors, always current.  step_host() writes its
    # results to the caller's pinned host buffers only; the first read of any of these afterwards (a checkpoint, the rollout
    # collector, policy_forward on sim.obs ...) mirrors them back to the device, on the current stream, once.
    def _refresh(self):
        h = self._host_out
        if h is not None:
            self._host_out = None
            # obs / rew / done / trunc are rewritten for every env by every step; terminal_obs / ep_return / ep_length only where an episode ended --
            # the caller's host buffers persist from step to step, so they hold the latest value of every env: whole-buffer copies are right for all seven
            for dst, src in zip((self._obs, self._rew, self._done, self._trunc, self._terminal_obs, self._ep_return, self._ep_length), h):
                if src is not None:
                    dst.copy_(src, non_blocking=True)

    obs, rew, done, trunc, terminal_obs, ep_return, ep_length = (
        _refreshed(n) for n in ("_obs", "_rew", "_done", "_trunc", "_terminal_obs", "_ep_return", "_ep_length"))

    def reset(self, mask=None, inject=None):
        """Reset all envs (mask None) or those with mask != 0.  Returns the (persistent) obs tensor."""
        m = _ptr(mask, torch.uint8, (self.n,), self.device)
        i = _ptr(inject, torch.float32, (self.n, NINJECT), self.device)
        _check(self.L.so100_reset(self.h, m, i, self.obs.data_ptr(), self._stream()), "so100_reset")
        return self.obs

    def step(self, actions, inject=None, rollout_row=None, terminal_obs=None):
        """actions: float32 [N,6] on the device.  Returns views of the handle's output tensors.
        rollout_row: optional float32 [N, obs_dim+10] row of a rollout buffer; reward/done are written into it.
        terminal_obs: optional float32 [N, obs_dim] destination of the terminal observations (default: self.terminal_obs)."""
        io = self._io
        io.rollout_row_dev = _ptr(rollout_row, torch.float32, (self.n, self.obs_dim + 10), self.device)
        io.act_dev = _ptr(actions, torch.float32, (self.n, 6), self.device)
        io.obs_dev = self.obs.data_ptr(); io.rew_dev = self.rew.data_ptr()
        io.done_dev = self.done.data_ptr(); io.trunc_dev = self.trunc.data_ptr()
        io.terminal_obs_dev = self.terminal_obs.data_ptr() if terminal_obs is None else _ptr(terminal_obs, torch.float32, (self.n, self.obs_dim), self.device)
        io.ep_return_dev = self.ep_return.data_ptr(); io.ep_length_dev = self.ep_length.data_ptr()
        io.inject_dev = _ptr(inject, torch.float32, (self.n, NINJECT), self.device)
        _check(self.L.so100_step(self.h, C.byref(io), self._stream()), "so100_step")
        return self.obs, self.rew, self.done, self.trunc

    def step_host(self, act, obs, rew, done, trunc, terminal_obs=None, ep_return=None, ep_length=None):
        """The same env step with every boundary buffer in PINNED HOST memory: the kernel reads the actions and writes its results
        over the host link itself -- one launch, no copy nodes (So100VecEnv's numpy path: 62 instead of 94 us per step at 4096 envs).
        The results are valid after the stream is synchronised; the handle's device-side obs / rew / done ... tensors are refreshed
        from these buffers lazily, on their next read (`_refresh`) -- so the buffers must stay alive and unmodified until then
        (So100VecEnv owns them; a following step_host() simply supersedes a mirror that nobody asked for: the numpy loop pays nothing)."""
        io = StepIO(_hptr(act, torch.float32, (self.n, 6)), _hptr(obs, torch.float32, (self.n, self.obs_dim)), _hptr(rew, torch.float32, (self.n,)),
                    _hptr(done, torch.uint8, (self.n,)), _hptr(trunc, torch.uint8, (self.n,)),
                    _hptr(terminal_obs, torch.float32, (self.n, self.obs_dim)), _hptr(ep_return, torch.float32, (self.n,)),
                    _hptr(ep_length, torch.int32, (self.n,)), None, None)
        _check(self.L.so100_step(self.h, C.byref(io), self._stream()), "so100_step")
        self._host_out = (obs, rew, done, trunc, terminal_obs, ep_return, ep_length)

    def set_policy(self, tensors):
        """tensors: dict name -> float32 device tensor (names: POLICY_TENSORS; SB3 keys: SB3_STATE_DICT_KEYS)."""
        shapes = policy_tensor_shapes(self.obs_dim)
        self._policy_tensors = {k: tensors[k] for k in POLICY_TENSORS}          # keep them alive
        self._pw = PolicyWeights(*[_ptr(tensors[k], torch.float32, shapes[k], self.device) for k in POLICY_TENSORS])
        self._pio = PolicyIO()

    def policy_forward(self, obs, act_env, step_counter, noise=None, act_raw=None, value=None, logp=None, rollout_row=None):
        """Fused SB3-MlpPolicy forward + sample + clip (+ rollout-row write): one launch on the current stream."""
        io = self._pio
        io.obs_dev = _ptr(obs, torch.float32, (self.n, self.obs_dim), self.device)
        io.noise_dev = _ptr(noise, torch.float32, (self.n, 6), self.device)
        io.act_env_dev = _ptr(act_env, torch.float32, (self.n, 6), self.device)
        io.act_raw_dev = _ptr(act_raw, torch.float32, (self.n, 6), self.device)
        io.value_dev = _ptr(value, torch.float32, (self.n,), self.device)
        io.logp_dev = _ptr(logp, torch.float32, (self.n,), self.device)
        io.rollout_row_dev = _ptr(rollout_row, torch.float32, (self.n, self.obs_dim + 10), self.device)
        _check(self.L.so100_policy_forward(self.h, C.byref(self._pw), C.byref(io), int(step_counter) & 0xFFFFFFFF, self._stream()), "so100_policy_forward")

    def rollout(self, rollout_buf, step_counter0, terminal_obs_chunk=None):
        """T = rollout_buf.shape[0] steps of {policy, sample, env step, buffer write} in one launch (persistent kernel).
        rollout_buf: float32 [T, N, obs_dim+10].  Uses / updates the handle's obs, rew, done, ... tensors.
        terminal_obs_chunk: optional float32 [T, N, obs_dim], receives the terminal observation wherever an episode ended."""
        T = rollout_buf.shape[0]
        io = RolloutIO(_ptr(rollout_buf, torch.float32, (T, self.n, self.obs_dim + 10), self.device), self.obs.data_ptr(), self.rew.data_ptr(),
                       self.done.data_ptr(), self.trunc.data_ptr(), self.terminal_obs.data_ptr(), self.ep_return.data_ptr(), self.ep_length.data_ptr(),
                       _ptr(terminal_obs_chunk, torch.float32, (T, self.n, self.obs_dim), self.device))
        _check(self.L.so100_rollout(self.h, C.byref(self._pw), C.byref(io), T, int(step_counter0) & 0xFFFFFFFF, self._stream()), "so100_rollout")

    def render(self, camera="end", width=None, height=None, envs=None, geoms=None, rgb=True, depth=False, segmentation=False,
               free_camera=None, out=None):
        """Ray-cast camera images of the envs' current state on the GPU (two launches on the current stream; DESIGN.md "Rendering").

        camera: "end" (the wrist camera end_point_camera, default 1080 x 1920, ROW 0 = BOTTOM of the view like the reference's
        mjr_readPixels) or "scene" (the viewer's free camera, default 800 x 800, rows top-down like Gymnasium's rgb_array).
        envs: None (all), a slice with step 1, or (begin, count).  geoms: None (the camera's default), an int of G_* bits or an
        iterable of names from GEOM_NAMES.  free_camera (scene camera only): dict with any of lookat (3), distance, azimuth,
        elevation, fovy (degrees).  out: a dict from an earlier call (same shapes) whose tensors are written in place -- the
        pixel-observation loop allocates nothing per step.
        Returns a dict of device tensors: "rgb" uint8 [count, H, W, 3], "depth" float32 [count, H, W] (camera-axis metres, sky 40),
        "segmentation" uint8 [count, H, W] (0 sky, 1 floor, 2 cube, 3..7 arm capsules, 8..15 finger pads).
        Memory: count * H * W * (3 rgb + 4 depth + 1 segmentation) bytes of output, plus a 448-byte scene record per env held by
        the handle (e.g. 4096 envs x 84 x 84 rgb: 87 MB; one 1080 x 1920 wrist frame with all three: 16.6 MB)."""
        if camera not in CAMERAS:
            raise So100Error(f"camera must be one of {sorted(CAMERAS)}, got {camera!r}")
        cam = CAMERAS[camera]
        dw, dh = K.END_CAMERA_SIZE if cam == CAM_END else K.SCENE_CAMERA_SIZE
        W, H = int(width or dw), int(height or dh)
        if envs is None:
            begin, count = 0, self.n
        elif isinstance(envs, slice):
            if envs.step not in (None, 1):
                raise So100Error("envs: only slices with step 1")
            begin, stop, _ = envs.indices(self.n)
            count = stop - begin
        else:
            begin, count = (int(v) for v in envs)
        if geoms is None:
            mask = 0
        elif isinstance(geoms, int):
            mask = geoms
        else:
            mask = 0
            for g in geoms:
                if g not in GEOM_NAMES:
                    raise So100Error(f"unknown geometry {g!r} (known: {sorted(GEOM_NAMES)})")
                mask |= GEOM_NAMES[g]
        fc = None
        if free_camera is not None:
            c = dict(K.SCENE_CAMERA)
            unknown = set(free_camera) - set(c)
            if unknown:
                raise So100Error(f"free_camera: unknown keys {sorted(unknown)}")
            c.update(free_camera)
            fc = (C.c_float * 7)(*[float(v) for v in c["lookat"]], float(c["distance"]), float(c["azimuth"]), float(c["elevation"]), float(c["fovy"]))
        want = {"rgb": (rgb, torch.uint8, (count, H, W, 3)), "depth": (depth, torch.float32, (count, H, W)),
                "segmentation": (segmentation, torch.uint8, (count, H, W))}
        res = {}
        for k, (on, dt, shape) in want.items():
            if not on:
                continue
            t = None if out is None else out.get(k)
            if t is None:
                t = torch.empty(shape, dtype=dt, device=self.device)
            _ptr(t, dt, shape, self.device)
            res[k] = t
        io = RenderIO(cam, W, H, begin, count, mask, C.cast(fc, C.c_void_p) if fc is not None else None,
                      res["rgb"].data_ptr() if "rgb" in res else None, res["depth"].data_ptr() if "depth" in res else None,
                      res["segmentation"].data_ptr() if "segmentation" in res else None)
        _check(self.L.so100_render(self.h, C.byref(io), self._stream()), "so100_render")
        return res

    def get_state(self):
        qpos = torch.empty(13, self.n, dtype=torch.float32, device=self.device)
        qvel = torch.empty(12, self.n, dtype=torch.float32, device=self.device)
        _check(self.L.so100_get_state(self.h, qpos.data_ptr(), qvel.data_ptr(), self._stream()), "so100_get_state")
        return qpos, qvel

    def set_state(self, qpos, qvel):
        _check(self.L.so100_set_state(self.h, _ptr(qpos, torch.float32, (13, self.n), self.device),
                                      _ptr(qvel, torch.float32, (12, self.n), self.device), self._stream()), "so100_set_state")

    def field_index(self, name):
        i = self.L.so100_state_field_index(name.encode())
        if i < 0:
            raise So100Error(f"unknown state field {name!r}")
        return i

    def field_names(self):
        return [self.L.so100_state_field_name(i).decode() for i in range(self.L.so100_num_state_fields())]

    # ---- sim checkpoint: the whole [field][N] state matrix as raw 32-bit words + the current
    # observation, beside the learner's own checkpoint (ref: main.py:227-232 saves only the SB3 zip).  Resuming is
    # bit exact: the Philox counters and the solver warm starts are rows of the matrix.
    def save_state(self, path):
        names = self.field_names()
        words = torch.stack([self.get_field(n, dtype=torch.int32) for n in names]).cpu().numpy()
        c = self.cfg
        np.savez(path, words=words, names=np.array(names), obs=self.obs.cpu().numpy(),
                 config=np.array([c.env_kind, c.num_envs, c.flags, c.solver_iters, c.contact_iters, c.frame_skip,
                                  c.max_episode_steps, c.seed, c.env_id_offset, self.envs_per_workgroup], dtype=np.int64))

    def load_state(self, path, allow_config_mismatch=False):
        with np.load(path, allow_pickle=False) as z:
            words, names, obs, conf = z["words"], [str(n) for n in z["names"]], z["obs"], z["config"]
        if int(conf[0]) != self.cfg.env_kind or int(conf[1]) != self.n:
            raise So100Error(f"checkpoint is for env kind {int(conf[0])} x {int(conf[1])} envs, this sim is kind {self.cfg.env_kind} x {self.n}")
        # resume is bit exact only under the configuration the checkpoint was taken with: refuse anything else
        c = self.cfg
        mine = [c.env_kind, c.num_envs, c.flags, c.solver_iters, c.contact_iters, c.frame_skip, c.max_episode_steps, c.seed, c.env_id_offset,
                self.envs_per_workgroup]
        labels = ["env_kind", "num_envs", "flags", "solver_iters", "contact_iters", "frame_skip", "max_episode_steps", "seed", "env_id_offset",
                  "envs_per_workgroup"]
        # (envs_per_workgroup follows from N and the device's CU count unless pinned: the pad-contact solve's summation order depends on it,
        #  so a resume is bit exact only under the same value; checkpoints of earlier versions do not carry it)
        diff = [f"{l}: checkpoint {int(a)} != sim {int(b)}" for l, a, b in zip(labels, conf, mine) if int(a) != int(b)]
        if len(conf) < len(mine):
            diff.append("envs_per_workgroup: not recorded in this (older) checkpoint")
        if diff and not allow_config_mismatch:
            raise So100Error("checkpoint was taken under a different configuration (" + "; ".join(diff) + "); pass allow_config_mismatch=True to load it anyway")
        missing = set(self.field_names()) - set(names)
        if missing and not allow_config_mismatch:
            raise So100Error(f"checkpoint lacks state fields {sorted(missing)} (written by an older version?); allow_config_mismatch=True zero-fills them")
        for n in sorted(missing):                           # older checkpoint, loaded on request: solver memory / statistics rows start from zero
            self.set_field(n, torch.zeros(self.n, dtype=torch.int32, device=self.device))
        for row, n in zip(words, names):
            if self.L.so100_state_field_index(n.encode()) >= 0:
                self.set_field(n, torch.from_numpy(row).to(self.device))
        self._host_out = None
        self._obs.copy_(torch.from_numpy(obs))

    def contacts_dropped(self):
        """int32 [N]: contacts dropped over the 16-record budget in the last env step (0 where the contact flags are off).  MuJoCo would keep
        them: an env that reports > 0 deviates from the reference model in that step (a jaw lying flat on the table)."""
        if (self.cfg.flags & (F_PADS_FLOOR | F_PADS_CUBE | F_LINKS_FLOOR | F_LINKS_CUBE)) == 0:
            return torch.zeros(self.n, dtype=torch.int32, device=self.device)
        return self.get_field("contact_stat", dtype=torch.int32) >> 8

    def bad_state_mask(self):
        """bool [N]: envs whose episode was ever ended by the non-finite state guard (NaN / inf action or state)."""
        return (self.get_field("bits", dtype=torch.int32) & B_BAD_STATE) != 0

    def get_field(self, name, dtype=torch.float32):
        out = torch.empty(self.n, dtype=dtype, device=self.device)
        _check(self.L.so100_get_field(self.h, self.field_index(name), out.data_ptr(), self._stream()), "so100_get_field")
        return out

    def set_field(self, name, value):
        assert value.element_size() == 4
        _check(self.L.so100_set_field(self.h, self.field_index(name), _ptr(value, value.dtype, (self.n,), self.device),
                                      self._stream()), "so100_set_field")


    # ---- model queries (include/so100_query.h): one launch each on the current stream, the state is only read ----------
    def _soa(self, t, k, what):
        """[M, k] -> the [k][M] array the kernels read, on the device (None stays None)"""
        if t is None:
            return None
        t = torch.as_tensor(t, dtype=torch.float32, device=self.device)
        if t.dim() != 2 or t.shape[1] != k:
            raise So100Error(f"{what}: want a [M, {k}] tensor, got {tuple(t.shape)}")
        return t.t().contiguous()

    def _problems(self, *soa):
        """M of a query: the given arrays' common length, or N where the handle's state is read"""
        ms = {t.shape[1] for t in soa if t is not None}
        if len(ms) > 1:
            raise So100Error(f"the arguments of a query hold different numbers of problems: {sorted(ms)}")
        return ms.pop() if ms else self.n

    def _out(self, M, *lead, dtype=torch.float32):
        return torch.empty(*lead, M, dtype=dtype, device=self.device)

    @staticmethod
    def _offset(offset):
        return None if offset is None else (C.c_float * 3)(*[float(v) for v in offset])

    @staticmethod
    def _six(x, name):
        """float[6] of six values or of one for all (a number of any kind, a sequence or a tensor)"""
        v = torch.as_tensor(x, dtype=torch.float32).reshape(-1).tolist()
        if len(v) not in (1, 6):
            raise So100Error(f"{name}: want 6 values or one for all, got {len(v)}")
        return (C.c_float*6)(*(v*6 if len(v) == 1 else v))

    def _stepping(self, what, mode, nsub, flags, solver_iters, contact_iters):
        """(mode, nsub, flags, solver_iters, contact_iters) as the io structs of trajectory(), derivatives() and closed_loop() hold them: the
        mode's number, and the handle's own value for each None"""
        if mode not in TRAJ_MODES:
            raise So100Error(f"{what}: mode must be one of {sorted(TRAJ_MODES)}, got {mode!r}")
        c = self.cfg
        return (TRAJ_MODES[mode], c.frame_skip if nsub is None else nsub, c.flags if flags is None else flags,
                c.solver_iters if solver_iters is None else solver_iters, c.contact_iters if contact_iters is None else contact_iters)

    def kinematics(self, q=None):
        """World poses from joint angles q [M, 6] (None: the handle's current joints, M = N).  Returns a dict of views, one row per problem:
        "xpos" [M, 6, 3] and "xmat" [M, 6, 3, 3] of the six link frames (link k = MuJoCo body k + 2), "ee" [M, 3] the reference's
        end-effector point, "cam_pos" [M, 3] and "cam_mat" [M, 3, 3] of the wrist camera."""
        qs = self._soa(q, 6, "q"); M = self._problems(qs)
        xpos, xmat, ee, cp, cm = self._out(M, 6, 3), self._out(M, 6, 9), self._out(M, 3), self._out(M, 3), self._out(M, 9)
        io = KinematicsIO(_optr(qs), xpos.data_ptr(), xmat.data_ptr(), ee.data_ptr(), cp.data_ptr(), cm.data_ptr())
        _check(self.L.so100_query_kinematics(self.h, C.byref(io), M, self._stream()), "so100_query_kinematics")
        return {"xpos": xpos.permute(2, 0, 1), "xmat": xmat.permute(2, 0, 1).unflatten(2, (3, 3)), "ee": ee.t(), "cam_pos": cp.t(),
                "cam_mat": cm.t().unflatten(1, (3, 3))}

    def jacobian(self, q=None, link=EE_LINK, offset=None):
        """mj_jac of the point at `offset` (3 values, link frame; None: the end-effector point on link 4, the frame origin on another link)
        of link `link`: "jacp" and "jacr" [M, 3, 6], world frame; columns of the joints behind the link are zero."""
        qs = self._soa(q, 6, "q"); M = self._problems(qs)
        jp, jr = self._out(M, 3, 6), self._out(M, 3, 6)
        off = self._offset(offset)
        io = JacobianIO(_optr(qs), link, C.cast(off, C.c_void_p) if off is not None else None, jp.data_ptr(), jr.data_ptr())
        _check(self.L.so100_query_jacobian(self.h, C.byref(io), M, self._stream()), "so100_query_jacobian")
        return {"jacp": jp.permute(2, 0, 1), "jacr": jr.permute(2, 0, 1)}

    def dynamics(self, q=None, v=None, qacc=None):
        """The arm's joint-space dynamics at q, v [M, 6] (q None: the handle's joints -- and, with v None too, its joint velocities; v None
        otherwise: zero): "M" [M, 6, 6] (armature included, as MuJoCo's qM), "bias" [M, 6] (qfrc_bias: Coriolis, centrifugal, gravity) and,
        with qacc [M, 6], "tau" = M qacc + bias."""
        qs, vs, acs = self._soa(q, 6, "q"), self._soa(v, 6, "v"), self._soa(qacc, 6, "qacc"); M = self._problems(qs, vs, acs)
        Mm, bias = self._out(M, 36), self._out(M, 6)
        tau = self._out(M, 6) if acs is not None else None
        io = DynamicsIO(*[_optr(t) for t in (qs, vs, acs, Mm, bias, tau)])
        _check(self.L.so100_query_dynamics(self.h, C.byref(io), M, self._stream()), "so100_query_dynamics")
        res = {"M": Mm.t().unflatten(1, (6, 6)), "bias": bias.t()}
        if tau is not None:
            res["tau"] = tau.t()
        return res

    def ik(self, target, q0=None, link=EE_LINK, offset=None, iters=IK_ITERS, damping=IK_DAMPING, tol=IK_TOL, max_step=IK_MAX_STEP):
        """Batched damped-least-squares IK: joint angles that put the point (link, offset: as in jacobian()) on target [M, 3], starting from
        q0 [M, 6] (None: the handle's current joints) and moving the joints 0..link inside their ranges.  Returns "q" [M, 6], "residual" [M]
        (metres), "iterations" [M] int32 and "converged" [M] uint8 (residual <= tol)."""
        ts, qs = self._soa(target, 3, "target"), self._soa(q0, 6, "q0"); M = self._problems(ts, qs)
        q, res, its, conv = self._out(M, 6), self._out(M), self._out(M, dtype=torch.int32), self._out(M, dtype=torch.uint8)
        off = self._offset(offset)
        io = IkIO(ts.data_ptr(), _optr(qs), link, C.cast(off, C.c_void_p) if off is not None else None, iters, damping,
                  tol, max_step, q.data_ptr(), res.data_ptr(), its.data_ptr(), conv.data_ptr())
        _check(self.L.so100_query_ik(self.h, C.byref(io), M, self._stream()), "so100_query_ik")
        return {"q": q.t(), "residual": res, "iterations": its, "converged": conv}

    def forward(self, qpos=None, qvel=None, ctrl=None, flags=None, solver_iters=FWD_SOLVER_ITERS, contact_iters=FWD_CONTACT_ITERS):
        """mj_forward for M states without stepping anything: the contacts, their forces and the constrained accelerations.  qpos [M, 13] and
        qvel [M, 12] as get_state() lays them out (both None: the handle's state, M = N; qvel alone None: zero), ctrl [M, 6] servo targets
        (None: the joint angles -- hold the pose), flags: SO100_F_* (None: the handle's).  Returns views, one row per problem: "qacc" and
        "qfrc_constraint" [M, 12] (arm 6, cube linear in the world frame, cube angular in the body frame), "ncon", "dropped" [M] int32,
        "residual" [M], "pad_force" [M, 8] (normal force per finger pad) and "contacts" = {"kind" (0 cube/floor, 1 pad/floor, 2 pad/cube, 3 proxy/floor,
        4 proxy/cube), "feat" [M, 20] int32 (feat -1 marks an empty slot), "pos" [M, 20, 3], "frame" [M, 20, 3, 3] (rows normal, t1, t2), "dist" [M, 20], "force" [M, 20, 3] (in the frame)}."""
        qs, vs, us = self._soa(qpos, 13, "qpos"), self._soa(qvel, 12, "qvel"), self._soa(ctrl, 6, "ctrl"); M = self._problems(qs, vs, us)
        i32 = dict(dtype=torch.int32)
        qacc, qfrc, ncon, drop, res, pf = self._out(M, 12), self._out(M, 12), self._out(M, **i32), self._out(M, **i32), self._out(M), self._out(M, 8)
        kind, feat, pos = self._out(M, FWD_MAXCON, **i32), self._out(M, FWD_MAXCON, **i32), self._out(M, FWD_MAXCON, 3)
        frame, dist, force = self._out(M, FWD_MAXCON, 9), self._out(M, FWD_MAXCON), self._out(M, FWD_MAXCON, 3)
        io = ForwardIO(*[_optr(t) for t in (qs, vs, us)], self.cfg.flags if flags is None else flags, solver_iters,
                       contact_iters, *[t.data_ptr() for t in (qacc, qfrc, ncon, drop, kind, feat, pos, frame, dist, force, pf, res)])
        _check(self.L.so100_query_forward(self.h, C.byref(io), M, self._stream()), "so100_query_forward")
        return {"qacc": qacc.t(), "qfrc_constraint": qfrc.t(), "ncon": ncon, "dropped": drop, "residual": res, "pad_force": pf.t(),
                "contacts": {"kind": kind.t(), "feat": feat.t(), "pos": pos.permute(2, 0, 1), "frame": frame.permute(2, 0, 1).unflatten(2, (3, 3)),
                             "dist": dist.t(), "force": force.permute(2, 0, 1)}}

    def trajectory(self, ctrl, qpos=None, qvel=None, mode="targets", nsub=None, flags=None, solver_iters=None, contact_iters=None):
        """Where M states end up under M open-loop control sequences, in one launch and without moving the simulation: ctrl [T, M, 6] holds, per
        control step, the servo targets in radians (mode "targets") or actions (mode "actions": targets = q at the start of the step + 0.075 a,
        the reach envs' law).  qpos [M, 13] and qvel [M, 12] as get_state() lays them out: an explicit state starts cold like a freshly reset env
        (qvel alone None: zero); both None: the handle's state with its warm starts, M = N -- the prediction of what step() would do next.
        nsub (substeps per control step), flags and the iteration counts default to the handle's own.  No task layer: no reward, TimeLimit,
        reset or RNG.  Returns views, row t = the state after control step t: "qpos" [T, M, 13], "qvel" [T, M, 12], "ee" [T, M, 3] (the
        end-effector point at that q), "ncon", "dropped", "sig" [T, M] int32 and "residual" [T, M] (what the contact_stat, contact_sig and
        solver_residual rows would hold after such a step) and "bad_step" [M] int32: the first step whose controls or resulting state are not
        finite (-1: none); from there on that problem's float rows are NaN and its int rows 0."""
        md, *knobs = self._stepping("trajectory", mode, nsub, flags, solver_iters, contact_iters)
        ctrl = torch.as_tensor(ctrl, dtype=torch.float32, device=self.device)
        if ctrl.dim() != 3 or ctrl.shape[2] != 6 or ctrl.shape[0] < 1:
            raise So100Error(f"ctrl: want a [T, M, 6] tensor, got {tuple(ctrl.shape)}")
        T = ctrl.shape[0]
        us = ctrl.permute(0, 2, 1).contiguous()
        qs, vs = self._soa(qpos, 13, "qpos"), self._soa(qvel, 12, "qvel"); M = self._problems(qs, vs, us[0])
        i32 = dict(dtype=torch.int32)
        qt, vt, et = self._out(M, T, 13), self._out(M, T, 12), self._out(M, T, 3)
        ncon, drop, sig, res, bad = self._out(M, T, **i32), self._out(M, T, **i32), self._out(M, T, **i32), self._out(M, T), self._out(M, **i32)
        io = TrajectoryIO(_optr(qs), _optr(vs), us.data_ptr(), md, T, *knobs, qt.data_ptr(), vt.data_ptr(), et.data_ptr(), None, None, ncon.data_ptr(), drop.data_ptr(), sig.data_ptr(), res.data_ptr(), bad.data_ptr())
        _check(self.L.so100_query_trajectory(self.h, C.byref(io), M, self._stream()), "so100_query_trajectory")
        return {"qpos": qt.permute(0, 2, 1), "qvel": vt.permute(0, 2, 1), "ee": et.permute(0, 2, 1), "ncon": ncon, "dropped": drop, "sig": sig,
                "residual": res, "bad_step": bad}

    def derivatives(self, ctrl, qpos=None, qvel=None, mode="targets", nsub=None, flags=None, eps=None, solver_iters=None, contact_iters=None):
        """The linearisation of one control step, MuJoCo's mjd_transitionFD, for M (state, control) pairs in one launch and without moving the
        simulation: the centred secant over +-eps of the step trajectory() takes with T = 1.  ctrl [M, 6], qpos [M, 13], qvel [M, 12], mode, nsub,
        flags and the iteration counts: as in trajectory() (None: the handle's own values; eps None: SO100_DERIV_EPS = 2^-6).  Tangent state
        x = (dq, v), 12 + 12 in MuJoCo's dof order: arm 6, cube linear 3 (world frame), cube angular 3 (body frame).  Returns "A" [M, 24, 24] =
        dx'/dx, "B" [M, 24, 6] = dx'/du, "qpos_next" [M, 13] and "qvel_next" [M, 12] (the unperturbed step) and "bad" [M] int32: 1 where the
        start, the controls or any of the 61 evaluations is not finite; that problem's float outputs are NaN.  With friction loss, limits or
        contacts the step is not smooth and the result depends on eps."""
        md, *knobs = self._stepping("derivatives", mode, nsub, flags, solver_iters, contact_iters)
        us, qs, vs = self._soa(ctrl, 6, "ctrl"), self._soa(qpos, 13, "qpos"), self._soa(qvel, 12, "qvel"); M = self._problems(qs, vs, us)
        A = torch.empty(M, DERIV_NX, DERIV_NX, dtype=torch.float32, device=self.device)
        B = torch.empty(M, DERIV_NX, DERIV_NU, dtype=torch.float32, device=self.device)
        qn, vn, bad = self._out(M, 13), self._out(M, 12), self._out(M, dtype=torch.int32)
        io = DerivativesIO(_optr(qs), _optr(vs), us.data_ptr(), md, *knobs, DERIV_EPS if eps is None else eps, A.data_ptr(), B.data_ptr(), qn.data_ptr(), vn.data_ptr(), bad.data_ptr())
        _check(self.L.so100_query_derivatives(self.h, C.byref(io), M, self._stream()), "so100_query_derivatives")
        return {"A": A, "B": B, "qpos_next": qn.t(), "qvel_next": vn.t(), "bad": bad}

    def lqr(self, A, B, lx, lxx, lu=None, luu=None, lux=None, *, nx=24, reg=0.0, alpha=1.0, u=None, u_lo=-1.0, u_hi=1.0, dx0=None):
        """The Riccati backward pass and the linear forward pass of one iLQR / LQR iteration for M problems in one launch (the handle's state is
        not read).  A [T, M, 24, 24] and B [T, M, 24, 6] as derivatives() returns them for T x M problems ordered t-major; nx = 24: the full
        tangent state, nx = 12: the arm block (tangent indices 0..5 and 12..17, read out of the same A and B).  With n = nx: lx [T + 1, M, n],
        lxx [T + 1, M, n, n] (row T: the terminal cost), lu [T, M, 6], luu [T, M, 6, 6], lux [T, M, 6, n] (None: zero), u [T, M, 6] nominal controls
        (None: no clamp; else u + du is kept in [u_lo, u_hi]), dx0 [M, n] (None: zero).  Returns "k" [T, M, 6], "K" [T, M, 6, n], "Vx0" [M, n],
        "Vxx0" [M, n, n], "dV" [M, 2] (the expected change of the model is alpha dV1 + alpha^2 dV2), "du" [T, M, 6] = alpha k + K dx (clamped with
        u), "dx" [T + 1, M, n] and "bad" [M] int32: -1, or the step whose Quu + reg I is not positive definite, or T for a non-finite input; a
        failed problem's float outputs are NaN."""
        io, M, out = self._lqr_io(A, B, lx, lxx, lu, luu, lux, nx, reg, alpha, u, u_lo, u_hi, dx0)
        _check(self.L.so100_query_lqr(self.h, C.byref(io), M, self._stream()), "so100_query_lqr")
        return out

    def lqr_reg(self, A, B, lx, lxx, lu=None, luu=None, lux=None, *, nx=24, reg=0.0, reg_min=1e-6, reg_max=1e10, reg_up=10.0, tries=8, alpha=1.0, u=None,
                u_lo=-1.0, u_hi=1.0, dx0=None):
        """lqr() with a regulariser per problem and the retry of a failed factor inside the launch.  reg: a float (every problem starts from it) or an
        [M] tensor (float32 on the device: read in place).  A problem whose Quu + reg I is not positive definite at some step runs its backward pass
        again under reg <- min(reg_max, max(reg_min, reg * reg_up)), up to `tries` passes and while reg < reg_max; the others are not held up by it
        and keep the reg they came with.  Returns lqr()'s dict -- for a problem that got through, bit for bit lqr()'s outputs under reg =
        reg_used -- plus "reg_used" [M] (the reg of the last pass run; NaN for a start that is negative or not finite) and "tries" [M] int32 (passes
        run: 0 for such a start).  "bad" is the last pass's."""
        start = None
        if isinstance(reg, torch.Tensor):
            if reg.dim() != 1:
                raise So100Error(f"reg: want a float or an [M] tensor, got {tuple(reg.shape)}")
            start = self._lqr_in(reg, (reg.shape[0],), "reg")
        base, M, out = self._lqr_io(A, B, lx, lxx, lu, luu, lux, nx, 0.0 if start is not None else reg, alpha, u, u_lo, u_hi, dx0)
        if start is not None and start.shape[0] != M:
            raise So100Error(f"reg: want a float or a [{M}] tensor, got {tuple(start.shape)}")
        out["reg_used"], out["tries"] = self._out(M), self._out(M, dtype=torch.int32)
        io = LqrRegIO(base, _optr(start), reg_min, reg_max, reg_up, tries, out["reg_used"].data_ptr(), out["tries"].data_ptr())
        _check(self.L.so100_query_lqr_reg(self.h, C.byref(io), M, self._stream()), "so100_query_lqr_reg")
        return out

    def reg_schedule(self, reg_used, best, *, keep=0, reg_min=1e-6, reg_max=1e10, reg_up=10.0, reg_down=0.1, out=None):
        """The next regulariser of each problem from the one its plan was made with (lqr_reg()'s "reg_used" [M]) and the line search's verdict
        (cost_select()'s "best" [M] int32), in one launch.  A problem improved where best is a candidate other than `keep` -- the index of the
        candidate that is the old plan (alpha = 0), -1 if there is none.  Improved: reg * reg_down, and 0 where that is under reg_min; not improved:
        min(reg_max, max(reg_min, reg * reg_up)).  out: the [M] tensor to write (reg_used itself is allowed), None: a new one.  Returns "reg" [M]
        and "improved" [M] uint8."""
        ru = torch.as_tensor(reg_used, dtype=torch.float32, device=self.device)
        if ru.dim() != 1 or ru.shape[0] < 1 or not ru.is_contiguous():
            raise So100Error(f"reg_used: want a contiguous [M] tensor, got {tuple(ru.shape)}")
        M = ru.shape[0]
        bs = torch.as_tensor(best, dtype=torch.int32, device=self.device).contiguous()
        if tuple(bs.shape) != (M,):
            raise So100Error(f"best: want a [{M}] tensor, got {tuple(bs.shape)}")
        if out is None:
            out = self._out(M)
        elif out.dtype != torch.float32 or tuple(out.shape) != (M,) or not out.is_contiguous() or out.device != ru.device:
            raise So100Error(f"out: want a contiguous float32 [{M}] tensor on {ru.device}")
        imp = self._out(M, dtype=torch.uint8)
        io = RegScheduleIO(ru.data_ptr(), bs.data_ptr(), keep, reg_min, reg_max, reg_up, reg_down, out.data_ptr(), imp.data_ptr())
        _check(self.L.so100_query_reg_schedule(self.h, C.byref(io), M, self._stream()), "so100_query_reg_schedule")
        return {"reg": out, "improved": imp}

    def _lqr_io(self, A, B, lx, lxx, lu, luu, lux, nx, reg, alpha, u, u_lo, u_hi, dx0):
        """lqr()'s arguments checked and packed: (the LqrIO, M, the outputs it points to)"""
        f32 = self._lqr_in
        A = torch.as_tensor(A, dtype=torch.float32, device=self.device)
        if A.dim() != 4 or A.shape[0] < 1 or A.shape[1] < 1:
            raise So100Error(f"A: want a [T, M, 24, 24] tensor, got {tuple(A.shape)}")
        if nx not in (12, 24):
            raise So100Error(f"lqr: nx must be 12 or 24, got {nx!r}")
        T, M, n = A.shape[0], A.shape[1], nx
        A, B = f32(A, (T, M, 24, 24), "A"), f32(B, (T, M, 24, 6), "B")
        lx, lxx = f32(lx, (T + 1, M, n), "lx"), f32(lxx, (T + 1, M, n, n), "lxx")
        lu, luu, lux = f32(lu, (T, M, 6), "lu"), f32(luu, (T, M, 6, 6), "luu"), f32(lux, (T, M, 6, n), "lux")
        u, dx0 = f32(u, (T, M, 6), "u"), f32(dx0, (M, n), "dx0")
        new = lambda *shape, **kw: torch.empty(*shape, dtype=kw.get("dtype", torch.float32), device=self.device)
        out = {"k": new(T, M, 6), "K": new(T, M, 6, n), "Vx0": new(M, n), "Vxx0": new(M, n, n), "dV": new(M, 2), "du": new(T, M, 6),
               "dx": new(T + 1, M, n), "bad": new(M, dtype=torch.int32)}
        io = LqrIO(n, T, *[_optr(t) for t in (A, B, lx, lxx, lu, luu, lux, u, dx0)], reg, alpha, u_lo, u_hi,
                   *[out[name].data_ptr() for name in ("k", "K", "Vx0", "Vxx0", "dV", "du", "dx", "bad")])
        io._inputs = (A, B, lx, lxx, lu, luu, lux, u, dx0)           # converted copies live as long as the io
        return io, M, out

    def closed_loop(self, u, qpos_ref, qvel_ref, K, k=None, *, alphas=(1.0,), nx=24, qpos=None, qvel=None, ref0=None, mode="targets", nsub=None, flags=None,
                    clamp=None, solver_iters=None, contact_iters=None):
        """Rollouts on the real dynamics under the feedback law c_t = u_t + alpha k_t + K_t (x_t (-) xref_t), for every step size in `alphas` at once:
        the nonlinear forward pass of iLQR with its line-search candidates, or LQR tracking of one plan from disturbed starts.  One launch, the
        simulation does not move.  u [T, M, 6] nominal controls and qpos_ref [T, M, 13], qvel_ref [T, M, 12] the nominal rollout, in trajectory()'s
        shapes (row t: the state AFTER step t -- trajectory()'s "qpos" and "qvel"; None with T = 1); K [T, M, 6, nx] and k [T, M, 6] (None: zero) as
        lqr() returns them; nx = 24 or 12 (the arm block).  qpos, qvel, mode, nsub, flags and the iteration counts: as in trajectory().  ref0 =
        (qpos [M, 13], qvel [M, 12]): the nominal state at the start; None: the start itself.  clamp = (lo, hi) keeps the controls applied inside.
        x (-) xref is the derivatives query's tangent difference.  Returns views with L = len(alphas): "u" [T, M, L, 6] the controls applied (the chosen
        candidate's is the next plan), "qpos" [T, M, L, 13], "qvel" [T, M, L, 12], "ee" [T, M, L, 3], "ncon", "dropped", "sig" [T, M, L] int32, "residual"
        [T, M, L] and "bad_step" [M, L] int32: trajectory()'s, firing also where a gain, nominal control or reference value read at that step is not finite."""
        md, *knobs = self._stepping("closed_loop", mode, nsub, flags, solver_iters, contact_iters)
        if nx not in (12, 24):
            raise So100Error(f"closed_loop: nx must be 12 or 24, got {nx!r}")
        u = torch.as_tensor(u, dtype=torch.float32, device=self.device)
        if u.dim() != 3 or u.shape[2] != 6 or u.shape[0] < 1:
            raise So100Error(f"u: want a [T, M, 6] tensor, got {tuple(u.shape)}")
        T = u.shape[0]
        al = [float(a) for a in alphas]
        L = len(al)
        if not 1 <= L <= CL_MAX_L:
            raise So100Error(f"closed_loop: want 1..{CL_MAX_L} alphas, got {L}")
        us = u.permute(0, 2, 1).contiguous()
        qs, vs = self._soa(qpos, 13, "qpos"), self._soa(qvel, 12, "qvel"); M = self._problems(qs, vs, us[0])

        def rows(t, kk, what):
            if t is None:
                return None
            t = torch.as_tensor(t, dtype=torch.float32, device=self.device)
            if tuple(t.shape) != (T, M, kk):
                raise So100Error(f"{what}: want a [{T}, {M}, {kk}] tensor, got {tuple(t.shape)}")
            return t.permute(0, 2, 1).contiguous()
        rq, rv = rows(qpos_ref, 13, "qpos_ref"), rows(qvel_ref, 12, "qvel_ref")
        r0q, r0v = (None, None) if ref0 is None else (self._soa(ref0[0], 13, "ref0 qpos"), self._soa(ref0[1], 12, "ref0 qvel"))
        self._problems(us[0], r0q, r0v)
        Kt, kt = self._lqr_in(K, (T, M, 6, nx), "K"), self._lqr_in(k, (T, M, 6), "k")
        i32 = dict(dtype=torch.int32)
        ML = M*L
        ut, qt, vt, et = self._out(ML, T, 6), self._out(ML, T, 13), self._out(ML, T, 12), self._out(ML, T, 3)
        ncon, drop, sig, res, bad = self._out(ML, T, **i32), self._out(ML, T, **i32), self._out(ML, T, **i32), self._out(ML, T), self._out(ML, **i32)
        alpha = (C.c_float*L)(*al)
        lo, hi = (0.0, 0.0) if clamp is None else clamp
        io = ClosedLoopIO(_optr(qs), _optr(vs), us.data_ptr(), md, T, *knobs, _optr(rq), _optr(rv), _optr(r0q), _optr(r0v), nx, _optr(kt), _optr(Kt), L, C.cast(alpha, C.c_void_p), int(clamp is not None), lo, hi,
                          ut.data_ptr(), qt.data_ptr(), vt.data_ptr(), et.data_ptr(), None, None, ncon.data_ptr(), drop.data_ptr(), sig.data_ptr(), res.data_ptr(),
                          bad.data_ptr())
        _check(self.L.so100_query_closed_loop(self.h, C.byref(io), M, self._stream()), "so100_query_closed_loop")
        cols = lambda t: t.unflatten(-1, (M, L))
        return {"u": cols(ut).permute(0, 2, 3, 1), "qpos": cols(qt).permute(0, 2, 3, 1), "qvel": cols(vt).permute(0, 2, 3, 1), "ee": cols(et).permute(0, 2, 3, 1),
                "ncon": cols(ncon), "dropped": cols(drop), "sig": cols(sig), "residual": cols(res), "bad_step": cols(bad)}

    def _cost(self, what, T, M, target, target_mode, link, offset, w_point, w_q, q_nom, w_v, w_u, w_terminal):
        """(so100_cost_def, what it points to, the target in the kernels' layout) of the cost arguments cost_terms() and cost_select() share"""
        if target_mode is None:
            target_mode = "cube" if target is None else ("fixed" if torch.as_tensor(target).dim() == 2 else "traj")
        if target_mode not in COST_TARGETS:
            raise So100Error(f"{what}: target_mode must be one of {sorted(COST_TARGETS)}, got {target_mode!r}")
        off = self._offset(offset)
        tg = None
        if target_mode != "cube":
            if target is None:
                raise So100Error(f"{what}: target_mode {target_mode!r} needs a target")
            tg = torch.as_tensor(target, dtype=torch.float32, device=self.device)
            want = (M, 3) if target_mode == "fixed" else (T, M, 3)
            if tuple(tg.shape) != want:
                raise So100Error(f"target: want a {list(want)} tensor, got {tuple(tg.shape)}")
            tg = tg.transpose(-1, -2).contiguous()
        d = CostDef(link, C.cast(off, C.c_void_p) if off is not None else None, COST_TARGETS[target_mode], w_point, self._six(w_q, "w_q"), self._six(q_nom, "q_nom"),
                    self._six(w_v, "w_v"), self._six(w_u, "w_u"), w_terminal)
        return d, off, tg

    def _rollouts(self, what, qpos, qvel, u, lead, bad_step, u_fallback, N):
        """The rollout arrays of cost_select(), cost_blend() and cost_refit() in the kernels' layout.  lead = (T, M, L) or (T, N K): qpos, qvel (None
        stays None) and u of shape lead + (k,) become [T][k][columns] -- closed_loop()'s and trajectory()'s views: no copy --, bad_step ([M, L], or
        N K values) [columns] int32 and u_fallback [T, N, 6] becomes [T][6][N]"""
        T, columns = lead[0], math.prod(lead[1:])
        soa = lambda t, k, name: None if t is None else self._shaped(t, (*lead, k), name).movedim(-1, 1).reshape(T, k, columns).contiguous()
        qs, vs, us = soa(qpos, 13, "qpos"), soa(qvel, 12, "qvel"), soa(u, 6, "u")
        if qs is None:
            raise So100Error(f"{what}: qpos is required")
        bs = None
        if bad_step is not None:
            bs = torch.as_tensor(bad_step, dtype=torch.int32, device=self.device)
            if len(lead) == 3 and tuple(bs.shape) != tuple(lead[1:]):
                raise So100Error(f"bad_step: want a [{lead[1]}, {lead[2]}] tensor, got {tuple(bs.shape)}")
            if bs.numel() != columns:
                raise So100Error(f"bad_step: want {columns} values, got {tuple(bs.shape)}")
            bs = bs.reshape(columns).contiguous()
        fb = None if u_fallback is None else self._shaped(u_fallback, (T, N, 6), "u_fallback").permute(0, 2, 1).contiguous()
        return qs, vs, us, bs, fb

    def cost_terms(self, qpos, qvel, u, *, nx=24, target=None, target_mode=None, link=EE_LINK, offset=None, w_point=1.0, w_q=0.0, q_nom=0.0, w_v=0.0,
                   w_u=0.0, w_terminal=1.0):
        """The Gauss-Newton quadratic model of the cost family of include/so100_query.h (so100_cost_def) along M trajectories, in one launch, as lqr()
        takes it.  qpos [T, M, 13], qvel [T, M, 12] (None: zero) and u [T, M, 6] in trajectory()'s shapes, row t the state AFTER step t.  The cost
        per state row: w_point |point - target|^2 + sum w_q (q - q_nom)^2 + sum w_v v^2, w_terminal times that at the last row, plus sum w_u u^2 per
        step; the point is (link, offset) as in jacobian().  target [M, 3] ("fixed"), [T, M, 3] ("traj") or None ("cube": the cube's position in
        the same row); target_mode None picks by the target's shape.  w_q, q_nom, w_v, w_u: 6 values or one for all.  nx = 24 or 12 (the arm
        block).  Returns "lx" [T + 1, M, nx], "lxx" [T + 1, M, nx, nx] (row 0 zero), "lu" [T, M, 6], "luu" [T, M, 6, 6]; a state row or control that is
        not finite gives NaN terms for that (step, problem)."""
        if nx not in (12, 24):
            raise So100Error(f"cost_terms: nx must be 12 or 24, got {nx!r}")
        u = torch.as_tensor(u, dtype=torch.float32, device=self.device)
        if u.dim() != 3 or u.shape[2] != 6 or u.shape[0] < 1 or u.shape[1] < 1:
            raise So100Error(f"u: want a [T, M, 6] tensor, got {tuple(u.shape)}")
        T, M = u.shape[0], u.shape[1]
        rows = lambda t, k, name: None if t is None else self._shaped(t, (T, M, k), name).permute(0, 2, 1).contiguous()      # trajectory()'s views: no copy
        qs, vs, us = rows(qpos, 13, "qpos"), rows(qvel, 12, "qvel"), rows(u, 6, "u")
        if qs is None:
            raise So100Error("cost_terms: qpos is required")
        d, keep, tg = self._cost("cost_terms", T, M, target, target_mode, link, offset, w_point, w_q, q_nom, w_v, w_u, w_terminal)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
        out = {"lx": new(T + 1, M, nx), "lxx": new(T + 1, M, nx, nx), "lu": new(T, M, 6), "luu": new(T, M, 6, 6)}
        io = CostTermsIO(C.pointer(d), _optr(tg), nx, T, qs.data_ptr(), _optr(vs), us.data_ptr(), *[out[k].data_ptr() for k in ("lx", "lxx", "lu", "luu")])
        _check(self.L.so100_query_cost_terms(self.h, C.byref(io), M, self._stream()), "so100_query_cost_terms")
        return out

    def cost_select(self, qpos, qvel, u, *, bad_step=None, u_fallback=None, target=None, target_mode=None, link=EE_LINK, offset=None, w_point=1.0, w_q=0.0,
                    q_nom=0.0, w_v=0.0, w_u=0.0, w_terminal=1.0):
        """The line search on closed_loop()'s output in one launch: the total cost of every candidate rollout, the cheapest candidate per problem and
        its controls as the next plan.  qpos [T, M, L, 13], qvel [T, M, L, 12] (None: zero), u [T, M, L, 6] (closed_loop()'s "qpos", "qvel", "u"),
        bad_step [M, L] int32 (None: no rollout failed), u_fallback [T, M, 6] (None: NaN): the plan kept where no candidate can be taken.  The cost
        arguments: as in cost_terms(); targets are per problem ([M, 3] or [T, M, 3]).  Returns "cost" [M, L] (+inf for a failed rollout), "best" [M]
        int32 (ties: the lowest index; -1: every candidate is +inf), "best_cost" [M] and "u_best" [T, M, 6]."""
        u = torch.as_tensor(u, dtype=torch.float32, device=self.device)
        if u.dim() != 4 or u.shape[3] != 6 or u.shape[0] < 1 or u.shape[1] < 1 or not 1 <= u.shape[2] <= CL_MAX_L:
            raise So100Error(f"u: want a [T, M, L, 6] tensor with L in 1..{CL_MAX_L}, got {tuple(u.shape)}")
        T, M, L = u.shape[0], u.shape[1], u.shape[2]
        qs, vs, us, bs, fb = self._rollouts("cost_select", qpos, qvel, u, (T, M, L), bad_step, u_fallback, M)
        d, keep, tg = self._cost("cost_select", T, M, target, target_mode, link, offset, w_point, w_q, q_nom, w_v, w_u, w_terminal)
        cost, best, bc, ub = self._out(M*L), self._out(M, dtype=torch.int32), self._out(M), self._out(M, T, 6)
        io = CostSelectIO(C.pointer(d), _optr(tg), T, L, qs.data_ptr(), _optr(vs), us.data_ptr(), _optr(bs), _optr(fb), cost.data_ptr(), best.data_ptr(),
                          bc.data_ptr(), ub.data_ptr())
        _check(self.L.so100_query_cost_select(self.h, C.byref(io), M, self._stream()), "so100_query_cost_select")
        return {"cost": cost.unflatten(0, (M, L)), "best": best, "best_cost": bc, "u_best": ub.permute(0, 2, 1)}

    def plan_sample(self, plan, K, sigma, *, seed=0, draw=0, id_offset=0, u_lo=-1.0, u_hi=1.0, qpos=None, qvel=None):
        """The candidates of a sampling planner in one launch, laid out as trajectory() reads them: K copies of each of the N plans [T, N, 6],
        perturbed by sigma (6 values or one for all; 0: never perturbed) times a standard normal and clamped to [u_lo, u_hi]; candidate 0 of every
        problem is the clamped plan itself.  The noise is a function of (seed, draw, id_offset + n, k, t, j) alone (include/so100_query.h): draw is
        the planner's call counter, id_offset the global index of problem 0.  qpos [N, 13] and qvel [N, 12] (optional): the start states to fan
        out.  Returns views of the SoA buffers, candidate (n, k) in row n K + k: "ctrl" [T, N K, 6] and, where given, "qpos" [N K, 13] and "qvel"
        [N K, 12] -- trajectory(res["ctrl"], res["qpos"], res["qvel"]) copies none of them."""
        return self._plan_sample("plan_sample", plan, K, sigma, False, seed, draw, id_offset, u_lo, u_hi, qpos, qvel)

    def _plan_sample(self, what, plan, K, sigma, per_entry, seed, draw, id_offset, u_lo, u_hi, qpos, qvel):
        """plan_sample() and plan_sample_tv() (per_entry: sigma is a [T, N, 6] tensor read on the device)"""
        plan = torch.as_tensor(plan, dtype=torch.float32, device=self.device)
        if plan.dim() != 3 or plan.shape[2] != 6 or plan.shape[0] < 1 or plan.shape[1] < 1:
            raise So100Error(f"plan: want a [T, N, 6] tensor, got {tuple(plan.shape)}")
        T, N = plan.shape[0], plan.shape[1]
        if not 1 <= K <= MPPI_MAX_K:
            raise So100Error(f"{what}: K must be in 1..{MPPI_MAX_K}, got {K!r}")
        if qvel is not None and qpos is None:
            raise So100Error(f"{what}: qvel needs qpos")
        ps = plan.permute(0, 2, 1).contiguous()
        if per_entry:
            sg = self._shaped(sigma, (T, N, 6), "sigma").permute(0, 2, 1).contiguous()
        qs, vs = self._soa(qpos, 13, "qpos"), self._soa(qvel, 12, "qvel")
        self._problems(ps[0], qs, vs)
        ctrl = self._out(N*K, T, 6)
        qr, vr = (None if qs is None else self._out(N*K, 13)), (None if vs is None else self._out(N*K, 12))
        IO = PlanSampleTvIO if per_entry else PlanSampleIO
        io = IO(ps.data_ptr(), sg.data_ptr() if per_entry else self._six(sigma, "sigma"), u_lo, u_hi, K, T, seed, draw, id_offset, _optr(qs), _optr(vs),
                ctrl.data_ptr(), _optr(qr), _optr(vr))
        _check(getattr(self.L, "so100_query_" + what)(self.h, C.byref(io), N, self._stream()), "so100_query_" + what)
        res = {"ctrl": ctrl.permute(0, 2, 1)}
        if qr is not None:
            res["qpos"] = qr.t()
        if vr is not None:
            res["qvel"] = vr.t()
        return res

    def cost_blend(self, qpos, qvel, u, K, *, temperature, bad_step=None, u_fallback=None, shift=0, tail="zero", target=None, target_mode=None, link=EE_LINK,
                   offset=None, w_point=1.0, w_q=0.0, q_nom=0.0, w_v=0.0, w_u=0.0, w_terminal=1.0):
        """The sampling planner's decision on trajectory()'s output in one launch: the total cost of each of the N K rollouts, per problem the
        soft-min weights exp(-(J - J_min) / temperature), normalised, over its K candidates, and the weighted mean of their controls as the next plan.
        qpos [T, N K, 13], qvel [T, N K, 12] (None: zero) and u [T, N K, 6] (the controls applied: plan_sample()'s "ctrl") in trajectory()'s
        shapes, candidate (n, k) in row n K + k; bad_step [N K] int32 (None: no rollout failed), u_fallback [T, N, 6] (None: NaN): the plan kept where
        every candidate failed.  shift = 1 moves the plan up one step, its last row 0 (tail "zero") or the blend's last row again ("hold").  The cost
        arguments: as in cost_terms(); targets are per problem.  Returns "cost" [N, K] (+inf for a failed rollout), "best" [N] int32 (-1: all failed),
        "best_cost" [N], "weight" [N, K], "ess" [N] (1 / sum w^2), "u_plan" [T, N, 6] and "u_first" [N, 6] (row 0 of the blend before the shift)."""
        u = torch.as_tensor(u, dtype=torch.float32, device=self.device)
        if u.dim() != 3 or u.shape[2] != 6 or u.shape[0] < 1 or not 1 <= K <= MPPI_MAX_K or u.shape[1] < K or u.shape[1] % K:
            raise So100Error(f"u: want a [T, N K, 6] tensor with K = {K!r} in 1..{MPPI_MAX_K}, got {tuple(u.shape)}")
        if tail not in BLEND_TAILS:
            raise So100Error(f"cost_blend: tail must be one of {sorted(BLEND_TAILS)}, got {tail!r}")
        T, NK = u.shape[0], u.shape[1]
        N = NK//K
        qs, vs, us, bs, fb = self._rollouts("cost_blend", qpos, qvel, u, (T, NK), bad_step, u_fallback, N)
        d, keep, tg = self._cost("cost_blend", T, N, target, target_mode, link, offset, w_point, w_q, q_nom, w_v, w_u, w_terminal)
        cost, best, bc, wt, ess = self._out(NK), self._out(N, dtype=torch.int32), self._out(N), self._out(NK), self._out(N)
        up, uf = self._out(N, T, 6), self._out(N, 6)
        io = CostBlendIO(C.pointer(d), _optr(tg), T, K, qs.data_ptr(), _optr(vs), us.data_ptr(), _optr(bs), _optr(fb), temperature, shift, BLEND_TAILS[tail],
                         cost.data_ptr(), best.data_ptr(), bc.data_ptr(), wt.data_ptr(), ess.data_ptr(), up.data_ptr(), uf.data_ptr())
        _check(self.L.so100_query_cost_blend(self.h, C.byref(io), N, self._stream()), "so100_query_cost_blend")
        return {"cost": cost.unflatten(0, (N, K)), "best": best, "best_cost": bc, "weight": wt.unflatten(0, (N, K)), "ess": ess, "u_plan": up.permute(0, 2, 1),
                "u_first": uf.t()}

    def plan_sample_tv(self, plan, K, sigma, *, seed=0, draw=0, id_offset=0, u_lo=-1.0, u_hi=1.0, qpos=None, qvel=None):
        """plan_sample() with a noise scale per entry, read on the device: sigma [T, N, 6] like plan (cost_refit()'s "sigma_out", passed on without a
        copy).  An entry with sigma 0 is never perturbed; one whose sigma is negative or not finite is NaN in every candidate but candidate 0.
        With sigma[t, n, j] = s[j] the result is plan_sample(plan, K, s)'s bit for bit.  Everything else, the returned views included: as in
        plan_sample()."""
        return self._plan_sample("plan_sample_tv", plan, K, sigma, True, seed, draw, id_offset, u_lo, u_hi, qpos, qvel)

    def cost_refit(self, qpos, qvel, u, K, E, *, alpha=0.0, plan=None, sigma=None, sigma_min, sigma_max, sigma_init, bad_step=None, u_fallback=None,
                   shift=0, tail="zero", target=None, target_mode=None, link=EE_LINK, offset=None, w_point=1.0, w_q=0.0, q_nom=0.0, w_v=0.0, w_u=0.0, w_terminal=1.0):
        """The cross-entropy planner's decision on trajectory()'s output in one launch: the total cost of each of the N K rollouts, per problem the E
        cheapest candidates (ordered by (cost, index); a failed rollout is never one), and the mean and the population standard deviation of their
        controls per (step, joint) as the next plan and the next sigma: mean = alpha plan + (1 - alpha) mu, sigma = clamp(alpha sigma + (1 - alpha) sd,
        sigma_min, sigma_max).  qpos, qvel, u, bad_step, u_fallback, shift, tail and the cost arguments: as in cost_blend().  plan and sigma [T, N, 6]:
        the old mean and sigma, both needed with alpha > 0.  sigma_min, sigma_max, sigma_init: 6 values or one for all; sigma_init is the last row of a
        shifted "sigma_out" and every row of a problem whose candidates all failed.  Returns "cost" [N, K], "best" [N] int32, "best_cost" [N] (cost_blend()'s
        bits), "elite" [N, E] int32 in ascending rank (-1 from slot n_elite on), "n_elite" [N] int32, "threshold" [N] (the last elite's cost), "mean"
        [T, N, 6], "sigma_out" [T, N, 6] and "u_first" [N, 6] (row 0 of the mean before the shift) -- views of the SoA buffers:
        plan_sample_tv(res["mean"], K, res["sigma_out"]) copies neither."""
        u = torch.as_tensor(u, dtype=torch.float32, device=self.device)
        if u.dim() != 3 or u.shape[2] != 6 or u.shape[0] < 1 or not 1 <= K <= MPPI_MAX_K or u.shape[1] < K or u.shape[1] % K:
            raise So100Error(f"u: want a [T, N K, 6] tensor with K = {K!r} in 1..{MPPI_MAX_K}, got {tuple(u.shape)}")
        if not 1 <= E <= K:
            raise So100Error(f"cost_refit: E must be in 1..K = {K}, got {E!r}")
        if tail not in BLEND_TAILS:
            raise So100Error(f"cost_refit: tail must be one of {sorted(BLEND_TAILS)}, got {tail!r}")
        T, NK = u.shape[0], u.shape[1]
        N = NK//K
        qs, vs, us, bs, fb = self._rollouts("cost_refit", qpos, qvel, u, (T, NK), bad_step, u_fallback, N)
        per = lambda t, name: None if t is None else self._shaped(t, (T, N, 6), name).permute(0, 2, 1).contiguous()
        pl, sg = per(plan, "plan"), per(sigma, "sigma")
        d, keep, tg = self._cost("cost_refit", T, N, target, target_mode, link, offset, w_point, w_q, q_nom, w_v, w_u, w_terminal)
        cost, best, bc = self._out(NK), self._out(N, dtype=torch.int32), self._out(N)
        el, ne, th = self._out(N*E, dtype=torch.int32), self._out(N, dtype=torch.int32), self._out(N)
        mean, so, uf = self._out(N, T, 6), self._out(N, T, 6), self._out(N, 6)
        io = CostRefitIO(C.pointer(d), _optr(tg), T, K, qs.data_ptr(), _optr(vs), us.data_ptr(), _optr(bs), _optr(fb), E, alpha, _optr(pl), _optr(sg),
                         self._six(sigma_min, "sigma_min"), self._six(sigma_max, "sigma_max"), self._six(sigma_init, "sigma_init"), shift, BLEND_TAILS[tail],
                         cost.data_ptr(), best.data_ptr(), bc.data_ptr(), el.data_ptr(), ne.data_ptr(), th.data_ptr(), mean.data_ptr(), so.data_ptr(), uf.data_ptr())
        _check(self.L.so100_query_cost_refit(self.h, C.byref(io), N, self._stream()), "so100_query_cost_refit")
        return {"cost": cost.unflatten(0, (N, K)), "best": best, "best_cost": bc, "elite": el.unflatten(0, (N, E)), "n_elite": ne, "threshold": th,
                "mean": mean.permute(0, 2, 1), "sigma_out": so.permute(0, 2, 1), "u_first": uf.t()}

    def _shaped(self, t, shape, name):
        """a float32 tensor of exactly `shape` on the handle's device, in whatever strides it has"""
        t = torch.as_tensor(t, dtype=torch.float32, device=self.device)
        if tuple(t.shape) != tuple(shape):
            raise So100Error(f"{name}: want a {list(shape)} tensor, got {tuple(t.shape)}")
        return t

    def _lqr_in(self, t, shape, name):
        """a contiguous float32 tensor of exactly `shape` on the handle's device, or None"""
        return None if t is None else self._shaped(t, shape, name).contiguous()


def learner_layout(obs_dim):
    """{name: (offset, shape)} of the flat parameter block of include/so100_learn.h (names: POLICY_TENSORS, PyTorch nn.Linear shapes) and
    its length.  Metadata only: answers without a GPU."""
    L = load()
    n = L.so100_learner_num_params(obs_dim)
    if n < 0:
        raise So100Error(f"the learner's network takes obs_dim 15 or 8, got {obs_dim}")
    return {k: (L.so100_learner_param_offset(obs_dim, k.encode()), shape) for k, shape in policy_tensor_shapes(obs_dim).items()}, n


class So100Learner(_Handle):
    """One handle of the on-device PPO learner (include/so100_learn.h): advantages and minibatch steps as raw launches on torch's CURRENT
    stream -- the stream So100Sim's launches go to, so a rollout that follows an update is ordered behind it.  The caller owns every
    tensor (parameters, Adam moments, buffers); the handle owns its partial-gradient scratch."""
    _create, _destroy = "so100_learner_create", "so100_learner_destroy"

    def __init__(self, obs_dim, device=None, max_minibatch=32768, gamma=0.99, gae_lambda=0.95, clip_range=0.2, vf_coef=0.5, max_grad_norm=0.5,
                 lr=3e-4, beta1=0.9, beta2=0.999, adam_eps=1e-5):
        device = _resolve_device(device, "the so100 learner", hip_only=True)
        self._open(device, LearnerConfig(obs_dim, device.index, max_minibatch, gamma, gae_lambda, clip_range, vf_coef, max_grad_norm, lr, beta1, beta2, adam_eps))
        self.obs_dim = obs_dim
        self.num_params = self.L.so100_learner_num_params(obs_dim)

    def advantages(self, rollout, last_obs, params, adv, ret, adv_stats, terminal_obs=None, rewards=None):
        """rollout: float32 [T, N, obs_dim+10] packed chunk (read only); terminal_obs: [T, N, obs_dim] or None (no TimeLimit bootstrap);
        writes adv [T, N], ret [T, N], adv_stats [2] (mean, unbiased std).  rewards: float32 [T, N] read in place of the chunk's reward
        column (normalize_rewards' output; so100_learner_advantages_r), or None."""
        T, N = rollout.shape[0], rollout.shape[1]
        f, d, o = torch.float32, self.device, self.obs_dim
        io = AdvantagesIO(_ptr(rollout, f, (T, N, o + 10), d), _ptr(terminal_obs, f, (T, N, o), d), _ptr(last_obs, f, (N, o), d),
                          _ptr(params, f, (self.num_params,), d), _ptr(adv, f, (T, N), d), _ptr(ret, f, (T, N), d), _ptr(adv_stats, f, (2,), d))
        if rewards is None:
            _check(self.L.so100_learner_advantages(self.h, C.byref(io), T, N, self._stream()), "so100_learner_advantages")
        else:
            _check(self.L.so100_learner_advantages_r(self.h, C.byref(io), _ptr(rewards, f, (T, N), d), T, N, self._stream()), "so100_learner_advantages_r")

    # ---- reward normalisation (SB3 VecNormalize's reward half; include/so100_learn.h "Reward normalisation") ------------------------------
    @staticmethod
    def reward_norm_workspace_bytes(T, N):
        n = load().so100_learner_reward_norm_workspace(T, N)
        if n < 0:
            raise So100Error(f"so100_learner_reward_norm_workspace failed ({n}): {load().so100_last_error().decode()}")
        return n

    def reward_norm_init(self, state):
        """state: float64 [3 + N] on the device <- mean 0, var 1, count 1e-4 and N zero running returns"""
        N = state.numel() - 3
        _check(self.L.so100_learner_reward_norm_init(self.h, _ptr(state, torch.float64, (3 + N,), self.device), N, self._stream()), "so100_learner_reward_norm_init")

    def _reward_norm_io(self, rollout, state, rewards, workspace, clip_reward, epsilon):
        T, N = rollout.shape[0], rollout.shape[1]
        d = self.device
        if workspace.dtype != torch.float64 or workspace.dim() != 1:
            raise So100Error("the reward-normalisation workspace is a 1-d float64 tensor (reward_norm_workspace_bytes(T, N) // 8 elements)")
        return RewardNormIO(_ptr(rollout, torch.float32, (T, N, self.obs_dim + 10), d), _ptr(state, torch.float64, (3 + N,), d),
                            _ptr(rewards, torch.float32, (T, N), d), _ptr(workspace, torch.float64, (workspace.numel(),), d), workspace.numel() * 8,
                            clip_reward, epsilon)

    def normalize_rewards(self, rollout, state, rewards, workspace, clip_reward=REWARD_NORM_CLIP, epsilon=REWARD_NORM_EPSILON):
        """rewards [T, N] float32 <- the chunk's reward column normalised as SB3's VecNormalize(norm_reward=True) does; state float64 [3 + N]
        (mean, var, count, running returns) is advanced by the chunk's T steps; workspace: float64, reward_norm_workspace_bytes(T, N) // 8
        elements.  The chunk is read only.  Three launches."""
        io = self._reward_norm_io(rollout, state, rewards, workspace, clip_reward, epsilon)
        _check(self.L.so100_learner_normalize_rewards(self.h, C.byref(io), rollout.shape[0], rollout.shape[1], self._stream()), "so100_learner_normalize_rewards")

    # ---- observation normalisation (SB3 VecNormalize's observation half, folded; include/so100_learn.h "Observation normalisation") ------------
    @staticmethod
    def obs_norm_workspace_bytes(T, N):
        n = load().so100_learner_obs_norm_workspace(T, N)
        if n < 0:
            raise So100Error(f"so100_learner_obs_norm_workspace failed ({n}): {load().so100_last_error().decode()}")
        return n

    def obs_norm_init(self, state):
        """state: float64 [2 obs_dim + 1] on the device <- mean 0, var 1, count 1e-4"""
        _check(self.L.so100_learner_obs_norm_init(self.h, _ptr(state, torch.float64, (2 * self.obs_dim + 1,), self.device), self._stream()), "so100_learner_obs_norm_init")

    def obs_norm_update(self, rollout, state, workspace):
        """state float64 [2 obs_dim + 1] (mean, var, count) absorbs the T*N observation rows of the packed chunk (read only); workspace: float64,
        obs_norm_workspace_bytes(T, N) // 8 elements.  Two launches."""
        T, N = rollout.shape[0], rollout.shape[1]
        d = self.device
        if workspace.dtype != torch.float64 or workspace.dim() != 1:
            raise So100Error("the observation-normalisation workspace is a 1-d float64 tensor (obs_norm_workspace_bytes(T, N) // 8 elements)")
        io = ObsNormIO(_ptr(rollout, torch.float32, (T, N, self.obs_dim + 10), d), _ptr(state, torch.float64, (2 * self.obs_dim + 1,), d),
                       _ptr(workspace, torch.float64, (workspace.numel(),), d), workspace.numel() * 8)
        _check(self.L.so100_learner_obs_norm_update(self.h, C.byref(io), T, N, self._stream()), "so100_learner_obs_norm_update")

    def obs_norm_fold(self, state, params, folded, norm, epsilon=OBS_NORM_EPSILON):
        """folded [P] <- params with both towers' first layers folded over (mean, 1/sqrt(var + epsilon)) of state, the other tensors copied;
        norm float32 [2 obs_dim] <- (mean, inv_std).  One launch."""
        f, d, P = torch.float32, self.device, self.num_params
        _check(self.L.so100_learner_obs_norm_fold(self.h, _ptr(state, torch.float64, (2 * self.obs_dim + 1,), d), epsilon, _ptr(params, f, (P,), d),
                                                  _ptr(folded, f, (P,), d), _ptr(norm, f, (2 * self.obs_dim,), d), self._stream()), "so100_learner_obs_norm_fold")

    def set_obs_norm(self, norm):
        """norm: float32 [2 obs_dim] on the device (obs_norm_fold's), read by every later advantages / minibatch step / update when its kernels
        run; None: off.  The handle keeps the tensor alive."""
        self._obs_norm = norm
        _check(self.L.so100_learner_set_obs_norm(self.h, _ptr(norm, torch.float32, (2 * self.obs_dim,), self.device)), "so100_learner_set_obs_norm")

    def _minibatch_io(self, rollout, idx, adv, ret, adv_stats, params, adam_m, adam_v, adam_step, stats, grads):
        """the so100_minibatch_io of both steps.  idx: an int64 [mb] tensor of flat indices t*N + n in any order, or an int mb for rows 0..mb-1"""
        T, N = rollout.shape[0], rollout.shape[1]
        f, d, o, P = torch.float32, self.device, self.obs_dim, self.num_params
        if isinstance(idx, int):
            mb, ip = idx, None
        else:
            mb = idx.numel(); ip = _ptr(idx, torch.int64, (mb,), d)
        return MinibatchIO(_ptr(rollout, f, (T, N, o + 10), d), T * N, ip, mb, adam_step, _ptr(adv, f, (T, N), d), _ptr(ret, f, (T, N), d),
                           _ptr(adv_stats, f, (2,), d), _ptr(params, f, (P,), d), _ptr(adam_m, f, (P,), d), _ptr(adam_v, f, (P,), d),
                           _ptr(stats, f, (4,), d), _ptr(grads, f, (P,), d))

    def minibatch_step(self, rollout, idx, adv, ret, adv_stats, params, adam_m, adam_v, adam_step, stats, grads=None):
        """One PPO gradient step on the rows idx of the packed chunk: an int64 [mb] tensor of flat indices t*N + n in any order, or an int mb
        for rows 0..mb-1.  params / adam_m / adam_v are updated in place; stats [4] (LEARNER_STATS) and optionally grads [P] are written."""
        io = self._minibatch_io(rollout, idx, adv, ret, adv_stats, params, adam_m, adam_v, adam_step, stats, grads)
        _check(self.L.so100_learner_minibatch_step(self.h, C.byref(io), self._stream()), "so100_learner_minibatch_step")

    @staticmethod
    def _terms(ent_coef, clip_range_vf, normalize_advantage, target_kl, lr):
        if normalize_advantage not in NORMALIZE_ADVANTAGE:
            raise So100Error(f"normalize_advantage must be one of {sorted(NORMALIZE_ADVANTAGE)}, got {normalize_advantage!r}")
        return PpoTerms(ent_coef, 0.0 if clip_range_vf is None else clip_range_vf, NORMALIZE_ADVANTAGE[normalize_advantage],
                        0.0 if target_kl is None else target_kl, -1.0 if lr is None else lr)

    def minibatch_step_ex(self, rollout, idx, adv, ret, adv_stats, params, adam_m, adam_v, adam_step, diag, ent_coef=0.0, clip_range_vf=None,
                          normalize_advantage="batch", target_kl=None, lr=None, update_state=None, grads=None):
        """minibatch_step with SB3's remaining loss terms (so100_ppo_terms): diag [8] (LEARNER_DIAG) is written instead of stats.
        clip_range_vf / target_kl None: off; lr None: the handle's.  update_state: int32 [2] {stopped, steps_applied}, zeroed by the caller
        at the start of an update; required with target_kl."""
        io = self._minibatch_io(rollout, idx, adv, ret, adv_stats, params, adam_m, adam_v, adam_step, None, grads)
        terms = self._terms(ent_coef, clip_range_vf, normalize_advantage, target_kl, lr)
        _check(self.L.so100_learner_minibatch_step_ex(self.h, C.byref(io), C.byref(terms), _ptr(diag, torch.float32, (8,), self.device),
                                                      _ptr(update_state, torch.int32, (2,), self.device), self._stream()), "so100_learner_minibatch_step_ex")

    def explained_variance(self, rollout, ret, out):
        """out [1] = 1 - var(ret - old_V)/var(ret) over the chunk (old_V: the value column of the packed chunk); NaN when var(ret) is 0"""
        T, N = rollout.shape[0], rollout.shape[1]
        f, d = torch.float32, self.device
        _check(self.L.so100_learner_explained_variance(self.h, _ptr(rollout, f, (T, N, self.obs_dim + 10), d), _ptr(ret, f, (T, N), d), T * N,
                                                       _ptr(out, f, (1,), d), self._stream()), "so100_learner_explained_variance")

    def shuffle(self, seed, epoch, n, out):
        """out: int64 [n] on the device = the permutation of (seed, epoch, n) that include/so100_learn.h specifies (1 <= n <= 2^30); one launch"""
        _check(self.L.so100_learner_shuffle(self.h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFF, n, _ptr(out, torch.int64, (n,), self.device),
                                            self._stream()), "so100_learner_shuffle")

    def update(self, rollout, last_obs, params, adam_m, adam_v, adv, ret, adv_stats, perm, out, *, epochs, mb, adam_step0, shuffle_seed, shuffle_epoch0=0,
               terminal_obs=None, terms=None, update_state=None, reward_norm=None):
        """One whole PPO update enqueued by one call (so100_learner_update): the advantages, the explained variance, then `epochs` epochs of
        {device shuffle, ceil(T*N/mb) minibatch steps numbered from adam_step0 + 1}.  adv / ret [T, N], adv_stats [2], perm int64 [T*N] and
        out float32 [UPDATE_OUT] are the caller's and are written: out[0:8] the last step's statistics (terms None: the plain step's four) or
        diagnostics, out[8] the explained variance, out[9:15] log_std as the last step read it.  terms: None for the plain step, or a dict of
        minibatch_step_ex's options (ent_coef, clip_range_vf, normalize_advantage, target_kl, lr); update_state: int32 [2], zeroed by the call,
        required with target_kl.  reward_norm: None, or a dict of normalize_rewards' arguments (state, rewards, workspace and optionally
        clip_reward, epsilon): the normalisation is enqueued first and the advantages read its output (so100_learner_update_r)."""
        T, N = rollout.shape[0], rollout.shape[1]
        f, d, o, P = torch.float32, self.device, self.obs_dim, self.num_params
        t = None
        if terms is not None:
            t = self._terms(terms.get("ent_coef", 0.0), terms.get("clip_range_vf"), terms.get("normalize_advantage", "batch"), terms.get("target_kl"), terms.get("lr"))
        io = UpdateIO(_ptr(rollout, f, (T, N, o + 10), d), _ptr(terminal_obs, f, (T, N, o), d), _ptr(last_obs, f, (N, o), d), T, N,
                      _ptr(params, f, (P,), d), _ptr(adam_m, f, (P,), d), _ptr(adam_v, f, (P,), d), _ptr(adv, f, (T, N), d), _ptr(ret, f, (T, N), d),
                      _ptr(adv_stats, f, (2,), d), _ptr(perm, torch.int64, (T * N,), d), epochs, mb, adam_step0, int(shuffle_epoch0) & 0xFFFFFFFF,
                      int(shuffle_seed) & 0xFFFFFFFFFFFFFFFF, C.pointer(t) if t is not None else None, _ptr(update_state, torch.int32, (2,), d),
                      _ptr(out, f, (UPDATE_OUT,), d))
        if reward_norm is None:
            _check(self.L.so100_learner_update(self.h, C.byref(io), self._stream()), "so100_learner_update")
        else:
            nio = self._reward_norm_io(rollout, reward_norm["state"], reward_norm["rewards"], reward_norm["workspace"],
                                       reward_norm.get("clip_reward", REWARD_NORM_CLIP), reward_norm.get("epsilon", REWARD_NORM_EPSILON))
            _check(self.L.so100_learner_update_r(self.h, C.byref(io), C.byref(nio), self._stream()), "so100_learner_update_r")
