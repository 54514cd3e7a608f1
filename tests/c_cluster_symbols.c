/* Link check of the clustering entry points (include/sourmash_amd.h, smh_index_cluster): each is called with the header's
 * prototype.  Needs no GPU: with one a four-node index is clustered through plain C, without one the device call returns 2;
 * the geometry, the budgets and the refusals of the arguments need no device either way. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sourmash_amd.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(void) {
  uint32_t lane_max = 0, tile = 0, search_tile = 0;
  smh_cluster_geometry(&lane_max, &tile);
  smh_search_geometry(NULL, &search_tile, NULL);
  CHECK(lane_max > 0 && tile == search_tile);
  const uint64_t def = smh_cluster_pair_budget();
  CHECK(def == (1ull << 27));
  smh_cluster_set_pair_budget(12345);
  CHECK(smh_cluster_pair_budget() == 12345);
  smh_cluster_set_pair_budget(0);
  CHECK(smh_cluster_pair_budget() == def);
  CHECK(smh_cluster_rounds() == 32);
  smh_cluster_set_rounds(5);
  CHECK(smh_cluster_rounds() == 5);
  smh_cluster_set_rounds(0);
  CHECK(smh_cluster_rounds() == 32);

  /* nodes {1, 2, 3, 4}, {3, 4, 5}, {5, 6}, {9}: a path 0 - 1 - 2 and a node alone */
  const int have = smh_device_available();
  const uint64_t held[4][4] = {{1, 2, 3, 4}, {3, 4, 5, 0}, {5, 6, 0, 0}, {9, 0, 0, 0}};
  KmerMinHash *nodes[4];
  for (int i = 0; i < 4; i++) {
    CHECK((nodes[i] = kmerminhash_new(0, 21, false, 42, UINT64_MAX, false)) != NULL);
    for (int k = 0; k < 4; k++)
      if (held[i][k]) kmerminhash_add_hash(nodes[i], held[i][k]);
  }
  SmhIndex *index = smh_index_new(nodes, 4);
  CHECK((index != NULL) == (have != 0));
  sourmash_err_clear();

  uint32_t cluster[4] = {9, 9, 9, 9}, rep[4] = {9, 9, 9, 9}, common[4] = {9, 9, 9, 9}, k = 9, sizes[4] = {9, 9, 9, 9};
  /* refused before the index or the device is looked at; nothing written */
  CHECK(smh_index_cluster(index, SMH_SEARCH_JACCARD, NAN, 0, SMH_CLUSTER_COMPONENTS, NULL, cluster, rep, NULL, &k) == 3);
  CHECK(smh_index_cluster(index, SMH_SEARCH_CONTAINMENT_NODE, 0.1, 0, SMH_CLUSTER_COMPONENTS, NULL, cluster, rep, NULL, &k) == 3);
  CHECK(smh_index_cluster(index, SMH_SEARCH_CONTAINMENT_QUERY, 0.1, 0, SMH_CLUSTER_GREEDY, NULL, cluster, rep, common, &k) == 3);
  CHECK(smh_index_cluster(index, 4, 0.1, 0, SMH_CLUSTER_GREEDY, NULL, cluster, rep, common, &k) == 3);
  CHECK(smh_index_cluster(index, SMH_SEARCH_JACCARD, 0.1, 0, SMH_CLUSTER_GREEDY + 1, NULL, cluster, rep, NULL, &k) == 3);
  CHECK(smh_index_cluster(index, SMH_SEARCH_JACCARD, 0.1, 0, SMH_CLUSTER_COMPONENTS, NULL, cluster, rep, common, &k) == 3);
  CHECK(smh_index_cluster(index, SMH_SEARCH_JACCARD, 0.1, 0, SMH_CLUSTER_COMPONENTS, NULL, NULL, rep, NULL, &k) == 1);
  CHECK(smh_index_cluster(index, SMH_SEARCH_JACCARD, 0.1, 0, SMH_CLUSTER_COMPONENTS, NULL, cluster, NULL, NULL, &k) == 1);
  CHECK(smh_index_cluster(index, SMH_SEARCH_JACCARD, 0.1, 0, SMH_CLUSTER_COMPONENTS, NULL, cluster, rep, NULL, NULL) == 1);
  CHECK(smh_index_sizes(NULL, sizes) == 1);
  CHECK(cluster[0] == 9 && rep[3] == 9 && common[0] == 9 && k == 9 && sizes[0] == 9);
  sourmash_err_clear();

  if (have) {
    CHECK(smh_index_sizes(index, sizes) == 0);
    CHECK(sizes[0] == 4 && sizes[1] == 3 && sizes[2] == 2 && sizes[3] == 1);
    /* Jaccard: (0, 1) = 2 / 5, (1, 2) = 1 / 4.  Over 0.2 the path is one component, represented by its largest node */
    CHECK(smh_index_cluster(index, SMH_SEARCH_JACCARD, 0.2, 0, SMH_CLUSTER_COMPONENTS, NULL, cluster, rep, NULL, &k) == 0);
    CHECK(k == 2 && cluster[0] == 0 && cluster[1] == 0 && cluster[2] == 0 && cluster[3] == 1);
    CHECK(rep[0] == 0 && rep[1] == 0 && rep[2] == 0 && rep[3] == 3);
    /* 1 / 4 is not over 0.25: the comparison is strict */
    CHECK(smh_index_cluster(index, SMH_SEARCH_JACCARD, 0.25, 0, SMH_CLUSTER_COMPONENTS, NULL, cluster, rep, NULL, &k) == 0);
    CHECK(k == 3 && cluster[1] == 0 && cluster[2] == 1 && cluster[3] == 2 && rep[2] == 2);
    /* greedy does not chain: 0 takes 1, and 2 -- adjacent to the member 1 only -- represents itself */
    CHECK(smh_index_cluster(index, SMH_SEARCH_JACCARD, 0.2, 0, SMH_CLUSTER_GREEDY, NULL, cluster, rep, common, &k) == 0);
    CHECK(k == 3 && cluster[0] == 0 && cluster[1] == 0 && cluster[2] == 1 && cluster[3] == 2);
    CHECK(rep[0] == 0 && rep[1] == 0 && rep[2] == 2 && rep[3] == 3);
    CHECK(common[0] == 4 && common[1] == 2 && common[2] == 2 && common[3] == 1);
    /* scores that put node 1 first: it takes both neighbours */
    const uint32_t scores[4] = {1, 7, 1, 1};
    CHECK(smh_index_cluster(index, SMH_SEARCH_MAX_CONTAINMENT, 0.4, 0, SMH_CLUSTER_GREEDY, scores, cluster, rep, common, &k) == 0);
    CHECK(k == 2 && rep[0] == 1 && rep[1] == 1 && rep[2] == 1 && cluster[2] == 0 && cluster[3] == 1);
    CHECK(common[0] == 2 && common[1] == 3 && common[2] == 1);
  } else {
    CHECK(smh_index_cluster(index, SMH_SEARCH_JACCARD, 0.1, 0, SMH_CLUSTER_COMPONENTS, NULL, cluster, rep, NULL, &k) == 2);
    CHECK(smh_index_cluster(index, SMH_SEARCH_JACCARD, 0.1, 0, SMH_CLUSTER_GREEDY, NULL, cluster, rep, common, &k) == 2);
    CHECK(cluster[0] == 9 && k == 9);
  }
  sourmash_err_clear();
  smh_index_free(index);
  for (int i = 0; i < 4; i++) kmerminhash_free(nodes[i]);
  printf("cluster abi client ok%s\n", have ? " (gpu)" : "");
  return 0;
}
