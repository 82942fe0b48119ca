/* asan_harness.c -- TEST INFRASTRUCTURE ONLY: the C oracle (cog_oracle.c) driven over the golden
 * trace scenarios in a plain executable, so that it can be built with
 * -fsanitize=address,undefined -- the equivalent of the reference's Debug build, which compiles
 * its core with -fsanitize=address,undefined (reference CMakeLists.txt:97-105).  The oracle
 * reproduces the reference's u8 wrap-around and its flat-DeckObs scans on
 * purpose; this run shows that none of it is undefined behaviour or an out-of-bounds access in
 * the restatement.
 *
 *   make -C oracle asan      -> oracle/_asan/harness_asan (sanitized) and oracle/_asan/harness (plain)
 *   oracle/_asan/harness_asan              one line per scenario: name, steps, resets, FNV-1a hash, flags
 *   oracle/_asan/harness_asan --selftest   a deliberate heap overread (the sanitizer must stop it)
 *   oracle/_asan/harness_asan --drivers    the scenarios of kDriverScen instead (tests/test_driver_sequences_cpu.py):
 *                                          auto-reset off (orc_set_autoreset) past every env's end, then
 *                                          reset_default and auto-reset on again; and host actions past
 *                                          their heads, clamped to (21, 21, 21, 6, 18) as the engine
 *                                          documents (COG_HAZ_BAD_ACTION), in a tenth of the slots
 *   oracle/_asan/harness_asan --corners    the scenarios of kCornerScen (tests/test_corners_cpu.py): max_steps 0
 *                                          (a reset with map generation for every env at every step) and 1,
 *                                          and one player (the turn passes back to the same player)
 *   oracle/_asan/harness_asan --offmask    host actions inside their heads that no mask allows (tests/test_offmask_cpu.py):
 *                                          every kind of tests/driver_cases.py's M op at max_steps 12 and 100000,
 *                                          1 to 4 players, the altered bytes from this file's own generator
 *
 * Scenarios: the reference trace sets of tests/golden/ref_traces (oracle/gen_golden.py traces():
 * the stored-mask driver with auto-resets, B-start seeds, 2 and 3 players, the selected-mask
 * loop), run as batches of n envs with seeds seed + i, every output record hashed after every step.
 * tests/test_oracle_asan.py checks that the sanitized build reports nothing and that its hashes
 * equal the plain build's.  Not used by the product, bench or smoke. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/cog_types.h"
#include "cog_oracle.h"

typedef struct {
  const char *name;
  uint32_t seed;
  uint8_t n_players, n_pieces;
  int difficulty;
  uint32_t max_steps, sampler_seed;
  int stored; /* 1: the current agent's stored mask (test_environment.cpp:97-98); 0: selected masks */
  int steps;
  size_t n;
  int no_reset; /* steps run with orc_set_autoreset(v, 0); then reset_default, the switch on, `steps` again */
  int clamped;  /* 1: a tenth of the (env, head) slots hold the head's clamp value, legal or not */
  int offmask;  /* 1 + the kind of kOffKinds: half the envs' actions altered inside their heads, no mask consulted */
} scenario;

static const scenario kScen[] = {
    {"C2shape_sel_medium", 12345, 4, 3, 1, 100000, 12345, 0, 1000, 16, 0, 0, 0},
    {"C3shape_sel_hard", 12345, 4, 3, 2, 100000, 12345, 0, 1000, 16, 0, 0, 0},
    {"stored_hard_ms30", 7, 4, 3, 2, 30, 7, 1, 1500, 16, 0, 0, 0},
    {"stored_medium_ms40_bstart", 70000, 4, 3, 1, 40, 70000, 1, 1500, 16, 0, 0, 0},
    {"c1like_2p_medium_sel", 0, 2, 3, 1, 100000, 0, 0, 20000, 1, 0, 0, 0},
    {"c1like_2p_medium_sto", 0, 2, 3, 1, 100000, 0, 1, 5000, 1, 0, 0, 0},
    {"p3_hard_sto_ms60", 300, 3, 3, 2, 60, 300, 1, 1500, 8, 0, 0, 0},
};
static const scenario kDriverScen[] = {
    {"stored_hard_ms8_noreset", 77, 4, 3, 2, 8, 77, 1, 120, 16, 1, 0, 0},
    {"sel_hard_ms8_noreset_3p", 77, 3, 3, 2, 8, 77, 0, 120, 16, 1, 0, 0},
    {"clamped_host_actions_sel", 77, 4, 3, 2, 8, 77, 0, 300, 16, 0, 1, 0},
    {"clamped_host_actions_sto", 78, 2, 3, 1, 12, 78, 1, 300, 16, 0, 1, 0},
};

static const scenario kCornerScen[] = {
    {"sto_hard_ms0_4p", 77, 4, 3, 2, 0, 77, 1, 40, 16, 0, 0, 0},
    {"sto_hard_ms1_4p", 77, 4, 3, 2, 1, 77, 1, 120, 16, 0, 0, 0},
    {"sel_hard_ms1_3p", 77, 3, 3, 2, 1, 77, 0, 120, 16, 0, 0, 0},
    {"sto_hard_1p_ms8", 77, 1, 3, 2, 8, 77, 1, 300, 16, 0, 0, 0},
    {"sel_hard_1p_1piece", 177, 1, 1, 2, 100000, 177, 0, 1000, 16, 0, 0, 0},
};

/* --offmask: kind k at max_steps 100000 and 12, the players rotating so that 1 to 4 meet both */
static const char *kOffKinds[9] = {"single", "replace", "all", "play", "special", "remove", "move", "shop", "sweep"};
#define N_OFF 18
static scenario gOffScen[N_OFF];
static char gOffName[N_OFF][48];

static void off_scenarios(void) {
  for (int q = 0; q < N_OFF; q++) {
    const int kind = q / 2, ends = q & 1;
    const int players = 1 + (kind + ends) % 4;
    snprintf(gOffName[q], sizeof gOffName[q], "offmask_%s_%dp_ms%d", kOffKinds[kind], players, ends ? 12 : 100000);
    const scenario sc = {gOffName[q], 909u + (uint32_t)q, (uint8_t)players, 3, 2, ends ? 12u : 100000u, 909u + (uint32_t)q,
                         0, 300, 16, 0, 0, 1 + kind};
    gOffScen[q] = sc;
  }
}

static uint32_t lcg_next(uint32_t *x) {
  *x = *x * 1664525u + 1013904223u;
  return *x >> 8;
}

/* the M op's kinds (tests/driver_cases.py offmask_actions) on one ActionData record */
static void off_alter(uint8_t *a, int kind, size_t i, int t, uint32_t *lcg) {
  static const uint8_t top[5] = {21, 21, 21, 6, 18};
  if (kind == 8) {                                         /* sweep: slot (i + t) mod 87 */
    int slot = (int)((i + (size_t)t) % 87u), k = 0;
    while (slot >= top[k]) slot -= top[k++];
    for (int j = 0; j < 5; j++) a[j] = j == k ? (uint8_t)(slot + 1) : 0;
    return;
  }
  const uint32_t hit = lcg_next(lcg) & 1u;
  const int head = kind >= 3 ? kind - 3 : (int)(lcg_next(lcg) % 5u);
  uint8_t v[5];
  for (int j = 0; j < 5; j++) v[j] = (uint8_t)(lcg_next(lcg) % (uint32_t)(top[j] + (kind == 2 ? 1 : 0)) + (kind == 2 ? 0u : 1u));
  if (!hit) return;
  for (int j = 0; j < 5; j++) {
    if (kind == 2) a[j] = v[j];                            /* all: every head uniform in 0..top */
    else if (j == head) a[j] = v[j];                       /* one head uniform in 1..top */
    else if (kind != 1) a[j] = 0;                          /* (replace keeps the other heads) */
  }
}

static uint64_t fnv(uint64_t h, const void *p, size_t b) {
  const uint8_t *c = (const uint8_t *)p;
  for (size_t k = 0; k < b; k++) h = (h ^ c[k]) * 0x100000001b3ull;
  return h;
}

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "--selftest")) {        /* the sanitizer is live: one heap overread */
    volatile uint8_t *p = (volatile uint8_t *)malloc(16);
    volatile int past = 16;
    const int v = p[past];
    free((void *)p);
    return v == 0x5a ? 3 : 4;
  }
  int bad = 0;
  const int drivers = argc > 1 && !strcmp(argv[1], "--drivers");
  const int corners = argc > 1 && !strcmp(argv[1], "--corners");
  const int offmask = argc > 1 && !strcmp(argv[1], "--offmask");
  if (offmask) off_scenarios();
  const scenario *list = drivers ? kDriverScen : corners ? kCornerScen : offmask ? gOffScen : kScen;
  const size_t n_list = drivers   ? sizeof(kDriverScen) / sizeof(kDriverScen[0])
                        : corners ? sizeof(kCornerScen) / sizeof(kCornerScen[0])
                        : offmask ? (size_t)N_OFF
                                  : sizeof(kScen) / sizeof(kScen[0]);
  for (size_t q = 0; q < n_list; q++) {
    const scenario *sc = &list[q];
    orc_vec *v = orc_create(sc->n);
    orc_sampler *s = orc_sampler_create(sc->n, sc->sampler_seed);
    uint8_t *masks = (uint8_t *)calloc(sc->n, COG_MASK_BYTES);
    if (!v || !s || !masks) return 2;
    if (orc_reset(v, sc->seed, sc->n_players, sc->n_pieces, sc->difficulty, sc->max_steps)) {
      printf("%s reset-failed\n", sc->name);
      bad = 1;
      continue;
    }
    uint64_t h = 0xcbf29ce484222325ull;
    long resets = 0;
    uint32_t lcg = sc->seed * 2654435761u + 1u;
    const int total = sc->no_reset ? 2 * sc->steps : sc->steps;
    if (sc->no_reset) orc_set_autoreset(v, 0);
    for (int t = 0; t < total; t++) {
      if (sc->no_reset && t == sc->steps) {                /* every env restarts; the switch back on */
        if (orc_reset_default(v)) bad = 1;
        orc_set_autoreset(v, 1);
      }
      const uint8_t *obs = (const uint8_t *)orc_obs(v);
      const uint8_t *agent = orc_agent_sel(v);
      if (sc->stored) {
        for (size_t i = 0; i < sc->n; i++)
          memcpy(masks + i * COG_MASK_BYTES,
                 obs + i * COG_OBS_BYTES + COG_OBS_PLAYER0 + (size_t)COG_OBS_PLAYER_STRIDE * agent[i] + COG_PD_MASK,
                 COG_MASK_BYTES);
        orc_sample(s, masks);
      } else {
        orc_sample(s, orc_sel(v));
      }
      if (sc->clamped) {
        static const uint8_t top[5] = {21, 21, 21, 6, 18};
        uint8_t *a = (uint8_t *)orc_sampler_actions(s);
        for (size_t i = 0; i < sc->n; i++)
          for (int k = 0; k < 5; k++) {
            lcg = lcg * 1664525u + 1013904223u;
            if ((lcg >> 16) % 10u == 0u) a[i * COG_ACTION_BYTES + (size_t)k] = top[k];
          }
      }
      if (sc->offmask) {
        uint8_t *a = (uint8_t *)orc_sampler_actions(s);
        for (size_t i = 0; i < sc->n; i++) off_alter(a + i * COG_ACTION_BYTES, sc->offmask - 1, i, t, &lcg);
      }
      orc_step(v, orc_sampler_actions(s));
      h = fnv(h, orc_obs(v), sc->n * COG_OBS_BYTES);
      h = fnv(h, orc_sel(v), sc->n * COG_MASK_BYTES);
      h = fnv(h, orc_rewards(v), sc->n * 4 * sizeof(float));
      h = fnv(h, orc_dones(v), sc->n);
      h = fnv(h, orc_agent_sel(v), sc->n);
      h = fnv(h, orc_infos(v), sc->n * COG_INFO_BYTES);
      h = fnv(h, orc_sampler_actions(s), sc->n * COG_ACTION_BYTES);
      for (size_t i = 0; i < sc->n; i++) resets += orc_dones(v)[i] ? 1 : 0;
    }
    uint32_t flags = 0;
    for (size_t i = 0; i < sc->n; i++) flags |= orc_flags(v, i);
    printf("%s %d %ld %016llx %02x\n", sc->name, sc->steps, resets, (unsigned long long)h, flags);
    fflush(stdout);
    free(masks);
    orc_sampler_destroy(s);
    orc_destroy(v);
  }
  return bad;
}
