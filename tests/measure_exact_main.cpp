// csrc/measure_exact.h alone, compiled by the host compiler (tests/test_cpu_measure.py builds it plainly and with -fsanitize=undefined):
// the 128-bit products and fraction comparisons the hull kernel decides its minimum width and minimum rectangle with.
// Reads lines from standard input and answers each with one line:
//   mul a b                 -> hi lo            the two words of a * b
//   width h1 len1 h2 len2   -> -1 | 0 | 1       the sign of h1^2 / len1 - h2^2 / len2
//   rect h1 t1 len1 h2 t2 len2 -> -1 | 0 | 1    the sign of h1 t1 / len1 - h2 t2 / len2
// and ends with "measure_exact: N lines ok".
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "measure_exact.h"

int main() {
  char op[16];
  int lines = 0;
  while (scanf("%15s", op) == 1) {
    uint64_t v[6] = {0, 0, 0, 0, 0, 0};
    const int n = !strcmp(op, "mul") ? 2 : (!strcmp(op, "width") ? 4 : (!strcmp(op, "rect") ? 6 : 0));
    if (n == 0) { fprintf(stderr, "measure_exact: unknown line %s\n", op); return 2; }
    for (int i = 0; i < n; ++i)
      if (scanf("%" SCNu64, &v[i]) != 1) { fprintf(stderr, "measure_exact: short line\n"); return 2; }
    if (n == 2) {
      const mx_u128 r = mx_mul(v[0], v[1]);
      printf("%" PRIu64 " %" PRIu64 "\n", r.hi, r.lo);
    } else if (n == 4) {
      printf("%d\n", mx_cmp_width(v[0], v[1], v[2], v[3]));
    } else {
      printf("%d\n", mx_cmp_rect(v[0], v[1], v[2], v[3], v[4], v[5]));
    }
    ++lines;
  }
  printf("measure_exact: %d lines ok\n", lines);
  return 0;
}
