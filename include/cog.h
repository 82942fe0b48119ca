/* cog.h -- C ABI of the MI355X-native City-of-Gold batched step engine (libcog_hip.so).
 *
 * This is the boundary a reference-side binding calls (see INTEGRATION.md for the pybind11 /
 * ctypes stubs).  Plain pointers and sizes only: no torch, numpy or HIP types.  Every entry
 * point returns an int status (COG_OK == 0) and never throws; cog_last_error() gives the
 * message of the last failing call on the calling thread.  A handle is single-threaded: calls
 * on one handle must not overlap.  Work is ordered on one HIP stream per handle.
 *
 * Record layouts (ObsData, ActionMask, ActionData, Info) are in cog_types.h and are
 * byte-identical to the reference's numpy structured views (reference include/api.h:67-161).
 *
 * Reference interface replaced by each group (reference file:line):
 *   cog_env_*      vec_cog_env<N> + py_vec_env<N>   include/vec_environment.h:10-81,
 *                                                   include/pybind/vectorized.h:25-105,185-214
 *   cog_sampler_*  vec_action_sampler<N> + py_vec_action_sampler<N>
 *                                                   include/vec_sampler.h:7-28,
 *                                                   include/pybind/vectorized.h:107-127,217-230
 *   cog_runner_*   ThreadedRunner<N> + py_threaded_runner<N>
 *                                                   include/runner.h:21-115,
 *                                                   include/pybind/vectorized.h:129-161,232-256
 */
#ifndef COG_H
#define COG_H

#include <stddef.h>
#include <stdint.h>

#include "cog_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define COG_API __attribute__((visibility("default")))
#else
#define COG_API
#endif

#define COG_ABI_VERSION 1

/* status codes */
#define COG_OK 0
#define COG_ERR_INVALID (-1)   /* bad argument: NULL handle, wrong batch length, ... */
#define COG_ERR_HIP (-2)       /* HIP runtime failure (message in cog_last_error) */
#define COG_ERR_MAPGEN (-3)    /* generate_map_failure (reference map.cpp:699-702) */
#define COG_ERR_NODEVICE (-4)  /* no usable gfx950 device: the engine never falls back to CPU */
#define COG_ERR_OOM (-5)       /* device or pinned-host allocation failed */

/* difficulty (reference include/constants.h:11) */
#define COG_EASY 0
#define COG_MEDIUM 1
#define COG_HARD 2

/* hazard flags reported per env by cog_env_hazards: reference UB or toolchain-dependent
 * behaviour that this engine defines */
/* generation gave up: after the reference's bounded attempts, or at a placement this engine cannot
 * hold where the reference, unbounded, would go on (a hex more than 62 cells from the origin, a 97th
 * piece, more than 1,008 hexes placed after a piece left the hex lattice; every generation seen past
 * one of these ends without a map in the reference too).  Raised as COG_ERR_MAPGEN "Failed to generate map". */
#define COG_HAZ_MAPGEN_FAIL 0x01u
#define COG_HAZ_ERASE_PAST 0x02u   /* map.cpp:727 erase past the end: GCC>=13 semantics used */
#define COG_HAZ_Q9_OOB 0x04u       /* map.cpp:347-352 write past player_locations: dropped */
#define COG_HAZ_Q24_CLAMP 0x08u    /* player.cpp:92 discard more than active: clamped */
#define COG_HAZ_GRID_OVER 0x10u    /* map wider than the 48x48 observation: rejected */
/* (GRID_OVER is the finished map's check alone, as the reference's finalize would overflow there; the
 * reset or the sync of the launch that meets it raises COG_ERR_MAPGEN "larger than the 48x48
 * observation grid".  Every other env of the batch holds its result; the flagged env's records and
 * state are unspecified until its next reset, which generates again whatever flags it carries; its
 * Info record, which a reset leaves alone, until its next episode end.) */
#define COG_HAZ_OOB_LOOKUP 0x20u   /* hex lookup outside the map: reads as mountain */
#define COG_HAZ_SCAN_OVER 0x40u    /* card scan past the DeckObs record */
#define COG_HAZ_B_START_LT4 0x80u  /* start piece B with < 4 players */
#define COG_HAZ_BAD_ACTION 0x100u  /* host action index past its head (reference: OOB access): clamped */

/* runner flags */
#define COG_RUNNER_DEVICE_VIEWS 0x1u  /* sync() does not refresh the host views (C5: outputs stay in HBM) */
#define COG_RUNNER_STORED_MASKS 0x2u  /* sample from the current agent's stored mask (full dynamics) */

typedef struct cog_env cog_env;
typedef struct cog_sampler cog_sampler;
typedef struct cog_runner cog_runner;

/* Persistent views.  Host views are pinned host memory updated in place by every synchronous
 * call (reference common.h:97-101 semantics: non-owning, persistent).  Device views are the
 * engine state itself, in HBM, same layouts. */
typedef struct cog_env_views {
  size_t n_envs;
  cog_obs_t *observations;                 /* [n] ObsData          */
  cog_action_mask_t *selected_action_masks;/* [n] ActionMask       */
  float *rewards;                          /* [n][4]               */
  uint8_t *dones;                          /* [n] bool             */
  uint8_t *agent_selection;                /* [n]                  */
  cog_info_t *infos;                       /* [n] Info             */
  void *d_observations;
  void *d_selected_action_masks;
  void *d_rewards;
  void *d_dones;
  void *d_agent_selection;
  void *d_infos;
} cog_env_views;

COG_API const char *cog_last_error(void);
COG_API int cog_abi_version(void);
COG_API int cog_device_count(int *out);
/* which persistent rollout kernel cog_runner_rollout launches for a shard of n envs with
 * n_players players, sampling the selected (stored_masks 0) or stored masks (measurement labels
 * only): 0 duo (k_env_rollout_duo + k_env_fixup), 1 wave (k_env_rollout), 2 pipe
 * (k_env_rollout_pipe), 3 trio (k_env_rollout_trio + k_env_fixup); $COG_ROLLOUT / $COG_TRIO
 * force one (cog_engine.hip rollout_kind).  One player selects like two (never the trio); a batch
 * reset with max_steps 0 takes what two players take, whatever its players (the trio's step ends
 * episodes at turn ends alone) */
COG_API int cog_rollout_kind(size_t n_envs, int n_players, int stored_masks);
/* the form of the trio launch (k_env_rollout_trio + k_env_fixup) over a shard of n_envs envs on
 * `device`, as cog_runner_rollout will launch it (read-only; computed by the launcher's own
 * helpers): envs per workgroup (64, or 32 under $COG_TRIO_EPW), workgroups = ceil(n_envs / epw),
 * lat 1 for the form taken by a launch of at most one workgroup per CU ($COG_TRIO_JT forces it),
 * wpc the workgroups per CU the dynamic LDS pad keeps (2 when workgroups > cus, $COG_TRIO_WPC =
 * 1..4 forces it; 0 when no pad is applied) and pad_lds its bytes (0 also where a CU's LDS over wpc
 * leaves no room beside the kernel's own: wpc 3 and 4), k_env_fixup's grid
 * (min(workgroups, cus)), and the CUs `device` exposes (256 where it cannot be asked) */
typedef struct cog_trio_form { int epw; unsigned workgroups; int lat; int wpc; size_t pad_lds; unsigned fixup_grid; unsigned cus; } cog_trio_form;
COG_API int cog_trio_form_of(size_t n_envs, int device, cog_trio_form *out);

/* ---- vectorized environment ------------------------------------------------------------ */
/* vec_cog_env<N>() (vec_environment.h:23-30): N default-constructed envs on `device`;
 * default params seed=std::random_device, 4 players, 3 pieces, EASY, 100000 max steps. */
COG_API int cog_env_create(size_t n_envs, int device, cog_env **out);
/* the same batch split over several GPUs of this process: shard k holds the contiguous envs
 * [first_k, first_k + count_k), the reference ThreadedRunner's block split (runner.h:33-38:
 * n / n_devices each, the last shard takes the remainder), with its own HIP stream.  A device
 * may be listed more than once (two shards, two streams, one GPU).  Seeds are seed + global
 * index, so every result is independent of the shard layout. */
COG_API int cog_env_create_multi(size_t n_envs, const int *devices, int n_devices, cog_env **out);
COG_API int cog_env_num_shards(const cog_env *env, int *out);
COG_API int cog_env_shard_info(const cog_env *env, int shard, size_t *first, size_t *count, int *device);
COG_API void cog_env_destroy(cog_env *env);
COG_API int cog_env_num_envs(const cog_env *env, size_t *out);
/* vec_cog_env::reset(seed, n_players, n_pieces, difficulty, max_steps, render)
 * (vec_environment.h:38-44): env i gets seed + i (u32).  Synchronous.  n_players 1..4 (one player
 * is a supported batch: the turn passes back to the same player); max_steps 0 ends every episode at
 * its first step.  A refused argument (COG_ERR_INVALID) launches nothing and leaves the handle alone. */
COG_API int cog_env_reset(cog_env *env, uint32_t seed, uint8_t n_players, uint8_t n_pieces,
                          int32_t difficulty, uint32_t max_steps, int32_t render);
/* vec_cog_env::reset() (vec_environment.h:32-36): keep params, continue each env's rng. */
COG_API int cog_env_reset_default(cog_env *env);
/* vec_cog_env::step(actions) (vec_environment.h:46-61) with n == num_envs host ActionData
 * records; auto-resets finished envs; host views refreshed before return.
 * An index past its head is clamped to the head's last entry and flagged COG_HAZ_BAD_ACTION.  An
 * index inside its head that the mask does not allow is executed as the reference executes it
 * (cog_env::step never reads the mask, environment.cpp:91-181: the first non-zero head of play,
 * play_special, move, get_from_shop, remove, on u8 counters that wrap around -- a card played from an
 * empty hand leaves 255 of it, a remove with none pending 255 pending removes, a purchase from an
 * empty shop slot 255 cards in it -- and a move in a closed direction leaves the map; the hazard flags
 * it can raise are COG_HAZ_Q24_CLAMP and COG_HAZ_OOB_LOOKUP).  It is not refused and not flagged
 * COG_HAZ_BAD_ACTION.  The same holds for cog_env_step_device and the runner's step. */
COG_API int cog_env_step(cog_env *env, const cog_action_t *actions, size_t n);
/* same, actions already in device memory (e.g. a sampler's device actions); single-shard envs */
COG_API int cog_env_step_device(cog_env *env, const void *d_actions, size_t n);
/* same, the actions produced by work queued on `stream` (a hipStream_t of the env's device, e.g.
 * torch.cuda.current_stream(); NULL is the null stream): the step is ordered after that work
 * (event + stream wait).  COG_NO_STREAM: no ordering (cog_env_step_device). */
#define COG_NO_STREAM ((void *)(intptr_t)-1)
COG_API int cog_env_step_device_stream(cog_env *env, const void *d_actions, size_t n, void *stream);
/* views (allocates + fills the pinned host views on first use).  Device pointers are set for
 * single-shard envs only; cog_env_shard_views gives shard k's device records and its slice of
 * the host views. */
COG_API int cog_env_get_views(cog_env *env, cog_env_views *out);
COG_API int cog_env_shard_views(cog_env *env, int shard, cog_env_views *out);
COG_API int cog_env_sync_host(cog_env *env);
/* OR of hazard flags over envs; per_env (n entries) may be NULL */
COG_API int cog_env_hazards(cog_env *env, uint32_t *flags_or, uint32_t *per_env);
COG_API int cog_env_clear_hazards(cog_env *env);
COG_API void *cog_env_stream(cog_env *env);     /* hipStream_t of shard 0 */
COG_API void *cog_env_shard_stream(cog_env *env, int shard);
/* ordering against a caller's stream on shard k's device (e.g. torch.cuda.current_stream();
 * NULL is the null stream):
 * wait_stream: engine work queued later on shard k runs after the work queued on `stream` so far;
 * signal_stream: work queued later on `stream` runs after the engine work queued on shard k */
COG_API int cog_env_wait_stream(cog_env *env, int shard, void *stream);
COG_API int cog_env_signal_stream(cog_env *env, int shard, void *stream);
/* after the caller wrote the env's device records (DLPack views / d_* pointers), ordered after
 * the work queued on `stream` so far (COG_NO_STREAM: none): the engine takes the records as they
 * now are, as the reference's views alias its live state (include/pybind/common.h:97-101) -- the
 * phase, resources and shop are read from the records anyway, and so are the decks by every launch
 * except a trio rollout that follows another one: that one starts from the compact deck image the
 * last one left, so once a trio rollout has run, deck writes are taken only after this call; the
 * selected and stored ActionMask records (0/1 bytes) and Info steps_taken also feed the engine's
 * private mirrors, which this rebuilds.  Host views are refreshed when the env has them.  Without
 * this call, writes to those records are not seen by the next step (see INTEGRATION.md "Device
 * views"). */
COG_API int cog_env_invalidate_device(cog_env *env, void *stream);

/* ---- state snapshots: save, restore and fork on the GPU ----------------------------------- */
/* An opaque copy of the complete state of every env of a handle, in device memory, one piece per
 * shard on the shard's device (about 4 KB per env: everything but the map observation, which a
 * restore encodes again).  The env's generator, seed, parameters and turn counter travel with it:
 * a restored env goes on exactly as the saved one would, under every driver.  Not in it: the
 * handle's auto-reset switch, samplers, timing.  A snapshot is independent of the handle it came
 * from (that handle may be destroyed) and may be restored any number of times, into any handle of
 * the same layout.
 *
 * cog_env_snapshot_create allocates a snapshot with env's layout (shard counts and devices).
 * cog_env_snapshot is enqueued on the shards' streams after their queued work (and after the work
 * queued on `stream`, COG_NO_STREAM: none) and returns without waiting; the handle's layout must
 * equal the snapshot's.  A snapshot of a handle that was never reset holds the default state.
 *
 * cog_env_restore: with d_src NULL env i takes snapshot env i (equal layouts).  With d_src, n_src
 * == num_envs indices in the env's device memory, of type src_kind, ordered after `stream`: env j
 * takes snapshot env d_src[j]; indices may repeat (a fork) and the snapshot may hold more or fewer
 * envs than the handle; both must be single-shard, on one device.  Every index is checked on the
 * device before anything is written, and the call waits for that check: an index outside the
 * snapshot, like every other refusal, returns COG_ERR_INVALID with the handle untouched.  A restore
 * ends as cog_env_invalidate_device does: host views (maps included) refreshed when the env has
 * them, the call complete on return.  The handle's batch parameters (players, max_steps) become
 * the snapshot's.  The sticky device status words are left alone (errors are reported by the call
 * that meets them); cog_env_hazards reads the per-env flags, which are restored. */
typedef struct cog_snapshot cog_snapshot;
#define COG_SRC_I32 0
#define COG_SRC_U32 1
#define COG_SRC_I64 2
COG_API int cog_env_snapshot_create(cog_env *env, cog_snapshot **out);
COG_API int cog_env_snapshot(cog_env *env, cog_snapshot *snap, void *stream);
COG_API int cog_env_restore(cog_env *env, const cog_snapshot *snap, const void *d_src, int src_kind, size_t n_src,
                            void *stream);
/* any out pointer may be NULL; bytes: device memory over all shards; n_players, max_steps: the
 * batch parameters of the handle at the last cog_env_snapshot (of its creation before) */
COG_API int cog_snapshot_info(const cog_snapshot *snap, size_t *n, int *n_shards, size_t *bytes, int *n_players,
                              uint32_t *max_steps);
COG_API int cog_snapshot_shard_info(const cog_snapshot *snap, int shard, size_t *count, int *device);
COG_API void cog_snapshot_destroy(cog_snapshot *snap);
/* diagnostics: re-run the map-observation encode (map.cpp:389-405) over all envs `iters`
 * times back to back; average device time per launch (HIP events).  Output is unchanged.
 * variant: 0 = production kernel, >0 = alternative implementations kept for A/B timing. */
COG_API int cog_env_time_encode(cog_env *env, int iters, int variant, double *ms_per_launch);
/* measurement: read + write bytes per second of the engine's device copy kernel (16-B loads and
 * stores, plain or non-temporal, 8 or 32 waves per CU: the fastest) over two `bytes` buffers on
 * `device`: the copy peak beside which the encode's HBM fraction is reported (BASELINE.md "a
 * measured copy-kernel peak") */
COG_API int cog_time_copy(int device, size_t bytes, int iters, double *gb_per_s);
/* measurement: read + write bytes per second of a stream with the encode's read:write mix (reads
 * `bytes`, writes 7 x `bytes`, coalesced, plain or non-temporal stores: the faster) on `device`:
 * the bandwidth peak of a kernel shaped like the map-observation encode */
COG_API int cog_time_stream_mix(int device, size_t bytes, int iters, double *gb_per_s);
COG_API int cog_env_device(const cog_env *env); /* device ordinal */
/* on (default): a finished env is reset inside the same step call, as vec_cog_env<N>::step does
 * (vec_environment.h:56-59).  off: cog_env::step semantics (environment.cpp:91-95) -- the env
 * stays done and later steps are dead steps until reset() */
COG_API int cog_env_set_autoreset(cog_env *env, int on);

/* ---- masked uniform random sampler ------------------------------------------------------- */
/* vec_action_sampler<N>(seed) (vec_sampler.h:9-13): sampler i seeded seed + i (seed a u32, the
 * sum not wrapped). */
COG_API int cog_sampler_create(size_t n_envs, uint64_t seed, int device, cog_sampler **out);
/* sharded like cog_env_create_multi (a runner needs the env's and the sampler's shards equal) */
COG_API int cog_sampler_create_multi(size_t n_envs, uint64_t seed, const int *devices, int n_devices,
                                     cog_sampler **out);
/* the batch is the block [first_index, first_index + n_envs) of a larger one (a rank's shard,
 * city_of_gold/shard.py): sampler i seeded seed + first_index + i, the sum in 64 bits as the
 * unsharded batch computes it (vec_sampler.h:9-13), so a sharded run samples the same actions for
 * every seed -- a u32 base of seed + first_index would wrap where the reference does not */
COG_API int cog_sampler_create_at(size_t n_envs, uint64_t seed, uint64_t first_index, const int *devices,
                                  int n_devices, cog_sampler **out);
COG_API int cog_sampler_num_shards(const cog_sampler *s, int *out);
COG_API void cog_sampler_destroy(cog_sampler *s);
/* vec_action_sampler::sample(masks) (vec_sampler.h:14-21): n == num_envs host ActionMask
 * records; host actions view refreshed before return. */
COG_API int cog_sampler_sample(cog_sampler *s, const cog_action_mask_t *masks, size_t n);
/* same, masks in device memory (e.g. an env's d_selected_action_masks); single-shard samplers */
COG_API int cog_sampler_sample_device(cog_sampler *s, const void *d_masks, size_t n);
/* Policy sampler (an addition: the reference samples uniformly only): masked categorical actions
 * from a batch of logits in device memory, one fused kernel.  Row i holds 92 logits in ActionMask
 * byte order (play 0..21, play_special 22..43, remove 44..65, move 66..72, get_from_shop 73..91),
 * float32 or bfloat16 (widened exactly), rows `ld` elements apart (ld >= 92, any value).  A mask
 * byte != 0 is valid.  Per head h = 0..4 the sampler's minstd_rand0 state advances once,
 * u = ((x - 1) >> 7) * 2^-24, and over the valid entries in float32: m = max l, w_j = exp(l_j - m),
 * Z = sum w, action = the smallest j whose inclusive prefix sum exceeds u * Z;
 * logp += (l_j - m) - log Z, entropy += log Z - sum w_j (l_j - m) / Z.  A head with no valid entry
 * gives 0 and contributes nothing.  COG_POLICY_GREEDY: the valid entry with the largest logit
 * (NaN as -inf, ties to the lowest index), no draws, state untouched.  A head whose valid entries
 * hold +inf, or nothing but -inf / NaN, takes the greedy choice and makes that env's logp and
 * entropy NaN: an illegal action is never produced.
 * Writes the first 8 bytes of each of the sampler's device ActionData records (as every sample
 * does; cog_sampler_device_actions) and d_logp / d_entropy (n floats each; either may be NULL);
 * the host actions view is not refreshed.  Single-shard samplers (and envs, on the same device,
 * env->n == n) only.  The kernel is ordered after the work queued on `stream` so far and, with the
 * env's masks, after the env's queued work; work queued later on `stream` runs after it.  The
 * call does not wait on the host.  d_masks: 16-byte aligned. */
#define COG_LOGITS_F32 0
#define COG_LOGITS_BF16 1
#define COG_MASKS_SELECTED 0   /* env's selected masks                */
#define COG_MASKS_STORED 1     /* env's current agent's stored mask   */
#define COG_MASKS_POINTER 2    /* d_masks: n ActionMask records        */
#define COG_POLICY_GREEDY 0x1u
typedef struct cog_policy_args {
  const void *d_logits; int logits_dtype; size_t ld;
  int mask_source; cog_env *env; const void *d_masks;
  float *d_logp; float *d_entropy;      /* may be NULL */
  uint32_t flags; void *stream;         /* caller's hipStream_t, or COG_NO_STREAM */
} cog_policy_args;
COG_API int cog_sampler_sample_policy(cog_sampler *s, const cog_policy_args *a);
/* Policy evaluator (an addition): the distribution cog_sampler_sample_policy draws from, seen from
 * the learner's side.  For n rows of new logits (92 per row in ActionMask byte order, float32 or
 * bfloat16 widened exactly, rows `ld` elements apart, ld >= 92) and the recorded pair of each row
 * -- its 128-byte ActionMask record (a byte != 0 is valid) and its action record, whose bytes 0..4
 * are play, play_special, remove, move, get_from_shop, records `action_stride` bytes apart -- the
 * forward gives the joint log-probability of the recorded actions and the entropy, the backward
 * their gradient with respect to the logits.  n is any size; no env or sampler handle is involved.
 * Forward, per head h (offset, size) = (0,22), (22,22), (44,22), (66,7), (73,19) with at least one
 * valid entry, over the valid entries in float32 (a NaN logit counts as -inf): m = max l,
 * d_j = l_j - m, w_j = exp(d_j), Z = sum w, p_j = w_j / Z, H = log Z - sum w_j d_j / Z; with a the
 * recorded action of the head, logp += d_a - log Z and entropy += H.  A head with no valid entry
 * contributes nothing and its action byte is ignored.
 * A row is bad when, for some non-empty head, the valid entries hold +inf or nothing but -inf / NaN
 * (the sampler's degenerate case), or the recorded action is no valid entry (a >= size, or its mask
 * byte is 0): its logp and entropy are NaN and its gradient row is all zeros whatever comes in.
 * A recorded action on a valid entry that holds -inf (or NaN) beside finite valid ones is no bad
 * row: p_a = 0, so logp is -inf, the entropy is that of the other entries and grad_a = g_lp.
 * Backward, with the incoming gradients g_lp[i], g_en[i] (float32; a NULL pointer counts as zeros):
 * for a valid entry j of a non-empty head of a good row
 *   grad_j = g_lp (1[j = a] - p_j) - g_en p_j (log p_j + H),   the g_en term 0 where p_j = 0,
 * and every other column (invalid entries, empty heads) is 0.  It recomputes the head terms from
 * the logits, masks and actions: the forward saves nothing.  d_grad_logits: n contiguous rows of
 * 92 in the logits' dtype (bfloat16: the head terms are computed in double, narrowed to float32 and
 * rounded to nearest even: float32 terms would round a few entries in 10^5 the other way, a whole
 * bfloat16 step off).  No atomics: the same inputs give the
 * same bits.  Each call is one kernel on `stream` of `device`; neither waits on the host, and
 * COG_NO_STREAM is refused (there is no stream of the library's own).  n == 0 launches nothing. */
typedef struct cog_policy_eval_args {
  size_t n;
  const void *d_logits; int logits_dtype; size_t ld;       /* COG_LOGITS_*, ld >= 92 elements        */
  const uint8_t *d_actions; size_t action_stride;          /* bytes between records, >= 5            */
  const void *d_masks;                                     /* n ActionMask records, 16-byte aligned  */
  float *d_logp; float *d_entropy;                         /* forward outputs; may be NULL           */
  const float *d_grad_logp; const float *d_grad_entropy;   /* backward inputs; NULL = zeros          */
  void *d_grad_logits;                                     /* backward output: n rows of 92, logits' dtype, 16-byte aligned */
  int device; void *stream;                                /* device ordinal; caller's hipStream_t (NULL: the null stream) */
} cog_policy_eval_args;
COG_API int cog_policy_evaluate(const cog_policy_eval_args *a);            /* forward  */
COG_API int cog_policy_evaluate_backward(const cog_policy_eval_args *a);   /* backward */
/* Per-seat generalised advantage estimation (an addition) over a time-major window of a turn-based
 * rollout: rows t = 0..T-1, envs i = 0..n-1.
 *   a = agents[t,i] & 3 is the seat whose action row t holds (agent_selection BEFORE step t);
 *   v = values[t,i] is that seat's value estimate at that state;
 *   dones[t,i] (a byte != 0 is done) and rewards[t,i,0..3] are the env's views AFTER step t.
 * rewards[t,i,:] is used only where dones[t,i] != 0 (the rewards view is stale between dones):
 * anywhere else it may hold anything, NaN included, without effect.  A done of any kind ends the
 * episode (a turn limit is not told from a win), and the row after it belongs to a new episode.
 * Each env keeps three numbers per seat p, walking t from T-1 down to 0: nv[p], the seat's next
 * value, starting at last_values[i,p] (0 when d_last_values is NULL): seat p's value at the state
 * after the last row; A[p], the advantage at the seat's next own row, starting at 0; R[p], the
 * reward pending for the seat, starting at 0.  At row t:
 *   1. if dones[t,i]: for all four seats, nv[p] = 0; A[p] = 0; R[p] = rewards[t,i,p];
 *   2. for a only: delta = R[a] + gamma nv[a] - v; A[a] = delta + gamma lam A[a];
 *      advantages[t,i] = A[a]; returns[t,i] = A[a] + v; nv[a] = v; R[a] = 0.
 * So gamma discounts per own decision of a seat, not per env row; the terminal reward lands
 * undiscounted on each seat's last row of the episode; a seat with no row in an episode contributes
 * nothing, and seats >= n_players never act.  This equals textbook GAE run on each seat's own rows
 * of each episode, bootstrapped with 0 after a done and with last_values at the window's end.
 * Rows of values / agents / dones are values_ld / agents_ld / dones_ld elements apart (>= n), rows
 * of rewards rewards_ld floats apart (>= 4 n, a multiple of 4, d_rewards 16-byte aligned);
 * d_last_values is n x 4 contiguous; the outputs are T x n contiguous.  float32 arithmetic, no
 * atomics: the same inputs give the same bits.  One kernel on `stream` of `device`; it does not wait
 * on the host, and COG_NO_STREAM is refused.  T == 0 or n == 0 launches nothing. */
typedef struct cog_gae_args {
  size_t T, n;
  const float *d_values; size_t values_ld;
  const uint8_t *d_agents; size_t agents_ld;
  const float *d_rewards; size_t rewards_ld;               /* in floats                              */
  const uint8_t *d_dones; size_t dones_ld;
  const float *d_last_values;                              /* may be NULL: zeros                     */
  float gamma, lam;
  float *d_advantages; float *d_returns;                   /* T rows of n, row stride n              */
  int device; void *stream;                                /* device ordinal; caller's hipStream_t (NULL: the null stream) */
} cog_gae_args;
COG_API int cog_policy_gae(const cog_gae_args *a);
/* Policy features (an addition): a network's input for every env of a single-shard handle, seen
 * from one seat, as two tensors in device memory written by one kernel.  The engine's records and
 * views are not touched.  With s the seat (its low two bits), np the env's n_players, player p's
 * cell (ix_p, iy_p) = (locx[p] - minx + 1, locy[p] - miny + 1), the [ix][iy] index of
 * observations.shared.map, and relative seat r = 1..3 the player (s + r) mod np when r < np, else
 * absent:
 *   vec[i][208], each value as a number (a byte b is float(b), no scaling):
 *     0 shared.phase; 1..3 shared.current_resources (the ACTING player's, whatever the seat);
 *     4..21 shared.shop; 22 np; 23, 24 own ix, iy; 25..129 the seat's own DeckObs bytes 0..104
 *     (draw, hand, active, played, discard: 21 types each); 130 + 26 (r - 1) + k for r = 1..3:
 *     k = 0 present (1 / 0), k = 1, 2 ix_r - ix_own, iy_r - iy_own, k = 3 cards in hand (sum of
 *     hand[0..20]), k = 4 cards in draw, k = 5..25 per card type the total over the five piles; all
 *     26 are 0 for an absent seat.
 *   local[i][10][W][W], W = 2 radius + 1: entry [c][a][b] is about the map cell
 *     (ix_own - radius + a, iy_own - radius + b): c = 0..5 map features 1..6 of the cell (what
 *     shared.map[ix][iy][1 + c] holds, taken from the engine's compact hex codes), c = 6, 7, 8: 1
 *     where relative seat 1, 2, 3 stands (players can share a cell: the channels are independent),
 *     c = 9: 1 where the cell lies inside the 48 x 48 grid; a cell outside it has 0 in all ten.
 * For an env with s >= np both rows are all zeros.  Sums are formed as integers; float32 values are
 * exact, bfloat16 ones their round to nearest even.  An env whose last reset failed
 * (COG_HAZ_MAPGEN_FAIL, COG_HAZ_GRID_OVER) gets unspecified rows; nothing outside its own records
 * is read.
 * seat_mode COG_SEAT_ACTING: s = agent_selection, read on the device; COG_SEAT_FIXED: s = seat
 * (0..3) for every env; COG_SEAT_POINTER: s = d_seats[i], n bytes in device memory.  radius 0..24;
 * dtype COG_LOGITS_F32 / COG_LOGITS_BF16, for both tensors; d_vec, d_local contiguous, aligned to
 * the element size (any element of a larger buffer may be the first).  The kernel runs on `stream`
 * (COG_NO_STREAM: the env's own) after the env's queued work, and the env's later work runs after
 * it; the call does not wait on the host.  n == 0 launches nothing. */
#define COG_SEAT_ACTING 0
#define COG_SEAT_FIXED 1
#define COG_SEAT_POINTER 2
#define COG_FEATURES_VEC 208
#define COG_FEATURES_CHANNELS 10
#define COG_FEATURES_MAX_RADIUS 24
typedef struct cog_features_args {
  int radius; int dtype;                                   /* 0..24; COG_LOGITS_F32 / COG_LOGITS_BF16 */
  int seat_mode; int seat; const uint8_t *d_seats;         /* COG_SEAT_*; FIXED: seat; POINTER: d_seats */
  void *d_vec; void *d_local;                              /* n x 208 and n x 10 x W x W elements     */
  void *stream;                                            /* caller's hipStream_t, or COG_NO_STREAM  */
} cog_features_args;
COG_API int cog_env_policy_features(cog_env *env, const cog_features_args *a);
COG_API cog_action_t *cog_sampler_actions(cog_sampler *s);   /* persistent host view */
COG_API void *cog_sampler_device_actions(cog_sampler *s);    /* device view (shard 0) */
COG_API void *cog_sampler_shard_device_actions(cog_sampler *s, int shard);
COG_API int cog_sampler_device(const cog_sampler *s);       /* device ordinal */
/* samples so far, and how many of them took the speculative sample of the env step before them
 * (env.step(actions) with this sampler's actions view samples the next actions from the masks it
 * leaves; sample() of that env's own mask view then needs no launch).  Diagnostics. */
COG_API int cog_sampler_spec_stats(const cog_sampler *s, uint64_t *samples, uint64_t *hits);

/* ---- runner: asynchronous sample/step on the env's streams (runner.h:81-100) ---------------- */
COG_API int cog_runner_create(cog_env *env, cog_sampler *s, size_t n_threads, uint32_t flags,
                              cog_runner **out);
COG_API void cog_runner_destroy(cog_runner *r);
COG_API size_t cog_runner_n_threads(const cog_runner *r);
COG_API int cog_runner_sample(cog_runner *r);    /* enqueue sample(selected masks) */
COG_API int cog_runner_step(cog_runner *r);      /* enqueue step(sampler actions); fuses a pending sample */
COG_API int cog_runner_sync(cog_runner *r);      /* wait; refresh host views unless DEVICE_VIEWS */
COG_API int cog_runner_rollout(cog_runner *r, int steps);   /* enqueue steps x (sample; step) */
/* rollout() steps per kernel launch: 1 = one launch per step; K > 1 = a persistent kernel runs
   K x (sample; step) per launch, storing every step's outputs as a single step does */
COG_API int cog_runner_set_chunk(cog_runner *r, int steps_per_launch);
COG_API int cog_runner_set_timing(cog_runner *r, int enable);
/* device time of the fused launches since enabled: HIP events bracket each step() launch and each
   rollout() batch on every shard's stream; the slowest shard's total; *launches = fused launches
   covered */
COG_API int cog_runner_kernel_time(cog_runner *r, double *total_ms, uint64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* COG_H */
