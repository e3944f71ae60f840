// so100_policy_tensors.h -- the one table of the policy's 13 tensors: X(name, rows, cols) in the order of so100_policy_weights
// (include/so100_sim.h) = PolicyWeights (so100_policy.hpp) = the flat parameter block of include/so100_learn.h, each tensor in
// nn.Linear layout weight[rows][cols].  rows / cols are expressions in HID, ACT_DIM and the observation width `od`, which the user of
// the table has in scope.  No includes, nothing of HIP: a plain host compiler takes it.  (lib.py's POLICY_TENSORS / policy_tensor_shapes say the
// same in Python; tests/test_learn_cpu.py holds them to the offsets and sizes the library derives from this table.)
#pragma once

#define SO100_POLICY_TENSORS(X) \
    X(pi_w0, HID, od)     X(pi_b0, HID, 1)     X(pi_w1, HID, HID)   X(pi_b1, HID, 1) \
    X(mu_w, ACT_DIM, HID) X(mu_b, ACT_DIM, 1)  X(log_std, ACT_DIM, 1) \
    X(vf_w0, HID, od)     X(vf_b0, HID, 1)     X(vf_w1, HID, HID)   X(vf_b1, HID, 1) \
    X(v_w, 1, HID)        X(v_b, 1, 1)

namespace so100 {
#define X(name, rows, cols) T_##name,
enum { SO100_POLICY_TENSORS(X) NUM_TENSORS };          // T_pi_w0 = 0 ... T_v_b = 12: a tensor's position in the structs and the block
#undef X
}
