/* cog_oracle.h -- TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement of the reference City-of-Gold vectorized environment
 * (reference include/vec_environment.h, include/sampler.h, include/vec_sampler.h,
 *  src/{environment,player,cards,map,geometry}.cpp), written in plain C.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this
 * library, and only as the checker / CPU baseline.  The product (gym-eldorado_amd/) never
 * links or calls it.
 *
 * Pinning: see oracle/README.md -- checked against the reference core compiled in this
 * container (oracle/_ref, hazard-free seeds) and the committed fixtures in tests/golden/.
 */
#ifndef COG_ORACLE_H
#define COG_ORACLE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* hazard flags (reference UB / toolchain-dependent behaviour) */
#define ORC_F_MAPGEN_FAIL 0x01u   /* generate_map_failure thrown (map.cpp:699-702) */
#define ORC_F_ERASE_PAST 0x02u    /* vector::erase past the end (map.cpp:727, Q5; GCC>=13 semantics) */
#define ORC_F_Q9_OOB 0x04u        /* add_players wrote past player_locations (map.cpp:347-352, Q9) */
#define ORC_F_Q24_CLAMP 0x08u     /* discard_cards n > n_active (player.cpp:92, Q24) */
#define ORC_F_GRID_OVER 0x10u     /* map wider than 49 cells: finalize would overflow (Q27) */
#define ORC_F_OOB_LOOKUP 0x20u    /* hex lookup outside hex_array */
#define ORC_F_SCAN_OVER 0x40u     /* card scan ran past the 105-byte DeckObs */
#define ORC_F_B_START_LT4 0x80u   /* start piece B with < 4 players (Q9 trigger) */

typedef struct orc_vec orc_vec;
typedef struct orc_sampler orc_sampler;

orc_vec *orc_create(size_t n);
void orc_destroy(orc_vec *v);
size_t orc_num_envs(const orc_vec *v);
/* vec_cog_env::reset(seed, ...) : env i reset with seed + i (u32).  Returns 0 or -1 on
 * generate_map_failure (envs before the failing one are reset, like the reference loop). */
int orc_reset(orc_vec *v, uint32_t seed, uint8_t n_players, uint8_t n_pieces,
              int difficulty, uint32_t max_steps);
int orc_reset_default(orc_vec *v);
int orc_reset_threaded(orc_vec *v, uint32_t seed, uint8_t n_players, uint8_t n_pieces,
                       int difficulty, uint32_t max_steps, int n_threads);
int orc_reset_default_threaded(orc_vec *v, int n_threads);   /* orc_reset_default over host threads */
/* vec_cog_env::step: actions = n ActionData records (64 B stride) */
int orc_step(orc_vec *v, const void *actions);
/* step only envs [lo, hi) */
int orc_step_range(orc_vec *v, const void *actions, size_t lo, size_t hi);
/* on (default): a finished env is reset inside the same step call (vec_environment.h:56-59).
 * off: cog_env::step alone (environment.cpp:91-95): the env stays done, later steps change nothing
 * of it, its records stand until orc_reset / orc_reset_default */
void orc_set_autoreset(orc_vec *v, int on);
void *orc_obs(orc_vec *v);            /* ObsData[n] */
void *orc_sel(orc_vec *v);            /* ActionMask[n] */
float *orc_rewards(orc_vec *v);       /* f32[n][4] */
uint8_t *orc_dones(orc_vec *v);       /* bool[n] */
uint8_t *orc_agent_sel(orc_vec *v);   /* u8[n] */
void *orc_infos(orc_vec *v);          /* Info[n] */
uint32_t orc_flags(const orc_vec *v, size_t i);   /* per-env sticky hazard flags */
void orc_clear_flags(orc_vec *v);
/* private state for debugging: 16 bytes per player + env scalars */
int orc_debug_state(const orc_vec *v, size_t i, uint32_t *out, size_t n_out);
/* counters of env i's last map generation (they decide nothing; a failed generation leaves what it
 * reached): [0] the largest candidate total add_random_piece enumerated, [1] the largest number of
 * placed pieces, [2] the recursion depth reached, [3] [4] the smallest and largest hex coordinate
 * (x or y) ever placed, [5] [6] the final dimx, dimy, [7..10] the start piece's cells in the final
 * hex_array: ix min, ix max, iy min, iy max, [11] hexes placed at a non-integer coordinate (a piece
 * connected to a travel piece whose failed placement left it reset at the origin: half a cell off
 * the lattice of the map).  Returns ORC_GEN_STATS. */
#define ORC_GEN_STATS 12
int orc_gen_stats(const orc_vec *v, size_t i, int32_t *out, size_t n_out);

/* Census of the draws that can be rejected: every draw r of uniform_int_distribution with
 * r >= 2147483645 - 31 (the top 32 values of minstd_rand0's range; a draw below them is accepted by
 * every range of this game) is counted as accepted or rejected (r >= k * (2147483645 / k) for a pile
 * of k; r == 2147483645 is rejected by every k), by site and by phase.  Counters are per env and per
 * sampler (nothing shared between the threads of orc_run_threaded) and decide nothing.
 * orc_census: out[18] = [phase][site][class], phase 0 inside orc_reset* / orc_reset_default*, 1 inside
 * a step, 2 inside the auto-reset that ends a step (its map generation and initial hands); class 0
 * accepted, 1 rejected. */
#define ORC_SITE_DECK 0     /* deck_draw: initial hands, turn ends, the draw specials */
#define ORC_SITE_ACTIVE 1   /* player_cards_from_active: discards and removes paid for a move */
#define ORC_SITE_MAP 2      /* generate / add_random_piece */
void orc_census_clear(orc_vec *v);
void orc_census(const orc_vec *v, size_t i, uint32_t *out);

orc_sampler *orc_sampler_create(size_t n, uint32_t seed);
orc_sampler *orc_sampler_create_at(size_t n, uint32_t seed, uint64_t first);   /* seeds seed + first + i */
void orc_sampler_destroy(orc_sampler *s);
void orc_sample(orc_sampler *s, const void *masks);   /* ActionMask[n] -> actions */
void orc_sample_range(orc_sampler *s, const void *masks, size_t lo, size_t hi);
/* the same from the stored mask of each env's current agent (the env's own, not the
 * agent_selections view, which a reset leaves stale): the full-dynamics driver */
void orc_sample_stored_range(orc_sampler *s, const orc_vec *v, size_t lo, size_t hi);
void *orc_sampler_actions(orc_sampler *s);            /* ActionData[n] */
uint32_t orc_sampler_state(const orc_sampler *s, size_t i);   /* sampler i's generator state */
/* out[4] = [a head with one candidate, a head with two or more][accepted, rejected] (see orc_census) */
void orc_sampler_census_clear(orc_sampler *s);
void orc_sampler_census(const orc_sampler *s, size_t i, uint32_t *out);

/* reference ThreadedRunner shape (runner.h:21-64): contiguous env blocks, one pinned worker
 * per block, per step "sample(selected masks); step(actions)" then a barrier.
 * Returns wall seconds for `steps` steps. */
double orc_run_threaded(orc_vec *v, orc_sampler *s, int steps, int n_threads);
/* `steps` x (sample; step) on the calling thread; 0, or -1 after a failed map generation */
int orc_run(orc_vec *v, orc_sampler *s, int steps, int stored);
/* the same loop; stored != 0 samples each env's current agent's stored mask instead */
double orc_run_threaded_masks(orc_vec *v, orc_sampler *s, int steps, int n_threads, int stored);

#ifdef __cplusplus
}
#endif
#endif
