// Host-only check of the bounce levels' chunk rounds (DESIGN.md §3.7;
// tests/test_sched_rounds.py).  lv_round_chunk (rtx_sched.h) is the function
// the level kernels call: workgroup b of G takes, as its n-th claim from its
// LDS counter, chunk (n / R) G R + b R + n mod R.  For every combination of
//   chunks in {0, 1, 7, 8, 9, 63, 64, 65, 1000, 120802}, G in {1, 2, 3, 256},
//   P (waves per workgroup) in {4, 8}, R in {1, 3, 8, 32, 4096},
//   lv_static % in {0, 37, 100}
// every workgroup draws n = 0, 1, ... as its P waves do (each wave stops at
// its first draw at or past S, the static part's size, so a workgroup makes
// exactly P such draws), and the program checks that
//   * every chunk below S is produced exactly once over the grid,
//   * no chunk at or above S is handed out,
//   * a workgroup's chunks increase strictly with n.
// Prints "cases <n> chunks <n> errors <n>"; exit status 1 on any error.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../raytracing_rb_amd/csrc/rtx_sched.h"

int main() {
  const uint32_t chunk_set[] = {0, 1, 7, 8, 9, 63, 64, 65, 1000, 120802};
  const uint32_t G_set[] = {1, 2, 3, 256}, P_set[] = {4, 8}, R_set[] = {1, 3, 8, 32, 4096}, pct_set[] = {0, 37, 100};
  static_assert(rtx::LV_ROUND_MAX == 4096, "the largest R checked is the option's bound");
  long cases = 0, handed = 0, errors = 0;
  for (uint32_t chunks : chunk_set)
    for (uint32_t G : G_set)
      for (uint32_t P : P_set)
        for (uint32_t R : R_set)
          for (uint32_t pct : pct_set) {
            const uint32_t S = rtx::lv_static_chunks(chunks, pct);
            std::vector<uint8_t> seen(S, 0);
            long bad = 0;
            for (uint32_t b = 0; b < G; b++) {
              uint32_t waves = P, n = 0;          // waves still claiming, the workgroup's counter
              bool first = true;
              uint32_t prev = 0;
              while (waves) {
                const uint32_t c = rtx::lv_round_chunk(n++, b, G, R);
                if (!first && c <= prev) bad++;   // strictly increasing in n
                first = false;
                prev = c;
                if (c >= S) {                     // that wave's static part is over: never handed out
                  waves--;
                  continue;
                }
                if (seen[c]++) bad++;             // twice
                handed++;
              }
            }
            for (uint32_t c = 0; c < S; c++)
              if (!seen[c]) bad++;                // never
            if (bad) fprintf(stderr, "chunks %u G %u P %u R %u pct %u: %ld errors\n", chunks, G, P, R, pct, bad);
            errors += bad;
            cases++;
          }
  printf("cases %ld chunks %ld errors %ld\n", cases, handed, errors);
  return errors ? 1 : 0;
}
