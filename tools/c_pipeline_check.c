/* Plain-C caller of the pipeline drivers (include/kaminpar_lp.h): runs
 * kmp_partition_deep_ex on rmat(14, 8, 42), k = 16, with default options and
 * with Jet + selection rebalancer + resident labels, then the same Jet
 * configuration through the ckaminpar-shaped shim's "jet" preset. Compiled
 * with gcc as C11 and linked against libkaminpar_lp.so; run by
 * tests/test_cpipeline_gpu.py::test_c_caller on a GPU.
 *
 * Prints one line per run: name, cut, FNV-1a 64 of the partition (as u32
 * little-endian bytes). Exit code 0 iff every call succeeded, the
 * default-options run equals plain kmp_partition_deep, and the preset run
 * equals the explicit-options run. */
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/kaminpar_lp.h"

static uint64_t fnv1a64(const uint32_t *part, uint32_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (uint32_t u = 0; u < n; ++u) {
    for (int b = 0; b < 4; ++b) {
      h ^= (part[u] >> (8 * b)) & 0xffu;
      h *= 0x100000001b3ull;
    }
  }
  return h;
}

#define FAIL(what)                                                             \
  do {                                                                         \
    fprintf(stderr, "FAIL: %s\n", what);                                       \
    return 1;                                                                  \
  } while (0)

int main(void) {
  const uint32_t k = 16;
  const double eps = 0.03;
  const uint64_t seed = 1;

  kmp_graph_t *g = kmp_gen_rmat(14, 8, 42);
  if (g == NULL) {
    FAIL("kmp_gen_rmat");
  }
  const uint32_t n = kmp_graph_n(g);
  uint32_t *plain = malloc(n * sizeof(uint32_t));
  uint32_t *part = malloc(n * sizeof(uint32_t));
  uint32_t *jet_part = malloc(n * sizeof(uint32_t));
  if (plain == NULL || part == NULL || jet_part == NULL) {
    FAIL("malloc");
  }

  /* default options == the plain entry point */
  const int64_t plain_cut = kmp_partition_deep(g, k, eps, seed, 5, 0, 0, 0, 0, plain);
  if (plain_cut < 0) {
    FAIL("kmp_partition_deep");
  }
  kmp_pipeline_opts_t o = kmp_pipeline_opts_default();
  kmp_pipeline_stats_t st;
  int64_t cut = kmp_partition_deep_ex(g, k, eps, seed, &o, part, &st);
  if (cut < 0) {
    FAIL("kmp_partition_deep_ex (default options)");
  }
  printf("default %" PRId64 " %016" PRIx64 "\n", cut, fnv1a64(part, n));
  if (cut != plain_cut || memcmp(part, plain, n * sizeof(uint32_t)) != 0) {
    FAIL("default options differ from kmp_partition_deep");
  }

  /* Jet with the selection rebalancer, labels resident */
  o.jet = 1;
  o.jet_fine.balancer = KMP_JET_BALANCER_SELECT;
  o.jet_coarse.balancer = KMP_JET_BALANCER_SELECT;
  o.resident = 1;
  const int64_t jet_cut = kmp_partition_deep_ex(g, k, eps, seed, &o, jet_part, &st);
  if (jet_cut < 0) {
    FAIL("kmp_partition_deep_ex (jet)");
  }
  printf("jet %" PRId64 " %016" PRIx64 "\n", jet_cut, fnv1a64(jet_part, n));
  if (st.jet_iterations == 0 || st.num_levels == 0 || st.level_sizes[0] != n) {
    FAIL("jet run reports no Jet iterations or no levels");
  }

  /* the same through the shim's preset */
  kaminpar_amd_t *shm = kaminpar_amd_create(1);
  if (shm == NULL) {
    FAIL("kaminpar_amd_create");
  }
  kaminpar_amd_reseed(shm, (int)seed);
  kaminpar_amd_copy_graph(shm, n, kmp_graph_xadj(g), kmp_graph_adjncy(g), kmp_graph_vwgt(g),
                          kmp_graph_adjwgt(g));
  kaminpar_amd_set_k(shm, k);
  kaminpar_amd_set_uniform_max_block_weights(shm, eps);
  if (kaminpar_amd_set_preset(shm, "nope") != -1 || kaminpar_amd_set_preset(shm, "jet") != 0) {
    FAIL("kaminpar_amd_set_preset");
  }
  cut = kaminpar_amd_compute_partition(shm, part);
  if (cut < 0) {
    FAIL("kaminpar_amd_compute_partition (preset jet)");
  }
  printf("preset %" PRId64 " %016" PRIx64 "\n", cut, fnv1a64(part, n));
  if (cut != jet_cut || memcmp(part, jet_part, n * sizeof(uint32_t)) != 0) {
    FAIL("preset jet differs from the explicit options");
  }

  kaminpar_amd_free(shm);
  kmp_graph_free(g);
  free(plain);
  free(part);
  free(jet_part);
  return 0;
}
