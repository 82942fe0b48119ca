// cog_feat.h -- the map features of a hex code, shared by the map-observation encode (cog_engine.hip)
// and the policy features (cog_policy.hip).  Included after a definition of DEV, inside namespace cog.
#pragma once

// Feature f of a hex code, f known at compile time after unrolling.  Code 0 (no hex) and NULL
// hexes (mountain / start, requirement 5) give all-zero features, like finalize's zero fill.
DEV uint32_t feat(uint32_t code, int f) {
  if (f == 0) return 0u;                                   // occupying player: never written (Q2)
  if (f == 6) return (code >> 6) & 1u;                     // is_end
  return (((code >> 3) & 7u) == (uint32_t)(f - 1)) ? (code & 7u) : 0u;
}
