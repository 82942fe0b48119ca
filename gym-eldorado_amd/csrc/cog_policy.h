// cog_policy.h -- internal interface between the C-ABI layer (cog_abi.cpp) and the policy sampler
// kernels (cog_policy.hip): masked categorical actions from a batch of logits, and the evaluator of
// recorded actions under new logits with its gradient, the per-seat advantage estimator, and the
// seat-relative observation tensors a network takes.  Not part of the public ABI (include/cog.h
// cog_sampler_sample_policy, cog_policy_evaluate, cog_policy_evaluate_backward, cog_policy_gae and
// cog_env_policy_features are).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace cog {

struct PolicyLaunch {
  size_t n;                          // envs
  const void *logits;                // [n] rows of >= 92 float32 / bfloat16 in ActionMask byte order
  int bf16;                          // 0: float32, 1: bfloat16
  size_t ld;                         // row stride in elements (>= 92)
  // env i's ActionMask record is mask_base + i * mask_stride + (agent ? agent[i] * 256 : 0), 16-B aligned:
  // the selected masks (stride 128), a caller's records (128), or the ObsData records' stored masks
  // (mask_base = obs + 16192 + 128, stride 17216, agent = the env's agent_selection bytes)
  const uint8_t *mask_base;
  size_t mask_stride;
  const uint8_t *agent;
  uint32_t *rng;                     // [n] the sampler's minstd_rand0 states (untouched when greedy)
  uint8_t *actions;                  // [n] ActionData records: the first 8 bytes of each are written
  float *logp, *entropy;             // [n] each, or null
  int greedy;
};

// 0, or -1 when the launch failed (hipGetLastError has the cause); n == 0 launches nothing
int launch_policy_sample(const PolicyLaunch &p, void *stream);

// the policy evaluator (include/cog.h cog_policy_evaluate / cog_policy_evaluate_backward)
struct PolicyEval {
  size_t n;                          // rows
  const void *logits;                // as PolicyLaunch
  int bf16;
  size_t ld;
  const uint8_t *actions;            // row i's recorded action bytes 0..4 at actions + i * action_stride
  size_t action_stride;              // >= 5
  const uint8_t *masks;              // [n] ActionMask records of 128 B, 16-B aligned
  float *logp, *entropy;             // forward: [n] each, or null
  const float *g_logp, *g_entropy;   // backward: [n] incoming gradients, null = zeros
  void *grad;                        // backward: [n] contiguous rows of 92 in the logits' dtype, 16-B aligned
};

// the forward or the backward kernel; 0, or -1 when the launch failed; n == 0 launches nothing
int launch_policy_eval(const PolicyEval &p, bool backward, void *stream);

// per-seat advantage estimation over a time-major window (include/cog.h cog_policy_gae)
struct TurnGae {
  size_t T, n;                       // rows, envs
  const float *values;               // [T] rows of n, values_ld floats apart (>= n)
  size_t values_ld;
  const uint8_t *agents;             // [T] rows of n seat bytes (low two bits), agents_ld bytes apart
  size_t agents_ld;
  const float *rewards;              // [T] rows of n x 4, rewards_ld floats apart (>= 4 n)
  size_t rewards_ld;
  const uint8_t *dones;              // [T] rows of n bytes (!= 0: done), dones_ld bytes apart
  size_t dones_ld;
  const float *last_values;          // [n][4], or null = zeros
  float gamma, lam;
  float *advantages, *returns;       // [T][n] contiguous
};

// 0, or -1 when the launch failed; T == 0 or n == 0 launches nothing
int launch_turn_gae(const TurnGae &p, void *stream);

// seat-relative observation tensors of a shard's envs (include/cog.h cog_env_policy_features)
constexpr int kFeatVec = 208;        // flat features per env
constexpr int kFeatChannels = 10;    // channels of the local map window
constexpr int kFeatMaxRadius = 24;
struct EnvPriv;
struct PolicyFeatures {
  size_t n;                          // envs
  const uint8_t *obs;                // DevState::obs: [n] ObsData records (read from byte 16128 on)
  const EnvPriv *priv;               // DevState::priv
  const uint8_t *agent;              // DevState::agent
  const uint8_t *cgrid;              // DevState::cgrid: [n] x 2304 hex codes
  const uint8_t *seats;              // [n] seat bytes (low two bits), or null: `seat`
  int seat;                          // 0..3 for every env, or -1: the acting seat (agent)
  int radius;                        // 0..24: the window is (2 radius + 1)^2 cells
  int bf16;                          // 0: float32, 1: bfloat16
  void *vec;                         // [n][208] contiguous, aligned to the element size
  void *local;                       // [n][10][W][W] contiguous, aligned to the element size
};

// 0, or -1 when the launch failed; n == 0 launches nothing
int launch_policy_features(const PolicyFeatures &p, void *stream);

}  // namespace cog
