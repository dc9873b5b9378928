// points_cluster.h -- the decisions of the KdTree's density clustering (lib_points_cluster.hip: sdfk_points_cluster*,
// sdfk_points_select*), written once for the device and the host: which candidates are within the radius, the saturating count
// and the core rule, the hook of an edge between two core points and its "changed" test, the root test and the bound on the
// rounds, the border point's choice among packed (d2, index) keys, the keep rule of select and the argument checks.  Plain C++
// outside hipcc, so that tests/cpp/points_cluster_host.cpp checks it as the kernels run it.  Contract: include/sdfkit_hip.h,
// "Point clouds: clusters".  Every quantity is an integer (d2 enters only through its bits in a key): nothing here depends on an
// order.
#pragma once
#include <cstdint>

#include "points_knn.h"

namespace sdfk_cluster {

using sdfk_knn::kKeyInf;

// ---- within ---------------------------------------------------------------------------------------------------------------------
// bound_key = pack_key(radius_d2_bound(radius), -1): the greatest key within the radius.  A candidate is within it iff its key is
// not above it -- d2 <= the bound on the bits of d2 (d2 >= 0), false for +inf and NaN, whatever the index: sdfk_points_radius_*'s
// predicate, the point itself and its duplicates included (d2 = 0).
SDFK_KNN_HD uint64_t bound_key_of(float radius) { return sdfk_knn::pack_key(sdfk_knn::radius_d2_bound(radius), -1); }
SDFK_KNN_HD bool reaches(uint64_t key, uint64_t bound_key) { return key <= bound_key; }

// ---- count and core -------------------------------------------------------------------------------------------------------------
SDFK_KNN_HD int32_t count_add(int32_t count) { return count == INT32_MAX ? count : count + 1; }   // (saturates: never wraps)
SDFK_KNN_HD bool is_core(int32_t count, int32_t min_points) { return count >= min_points; }

// ---- the label rounds: parent[i] <= i always, and parent[i] names a core point of i's cluster ------------------------------------
// The edge between two core points whose parents are pi and pj: nothing to do when they agree; otherwise the lower parent is
// offered, by atomicMin, to the parent of the higher one.
SDFK_KNN_HD bool hook_edge(int32_t pi, int32_t pj, int32_t* at, int32_t* offered)
{
    if (pi == pj) return false;
    *at = pi > pj ? pi : pj;
    *offered = pi > pj ? pj : pi;
    return true;
}
SDFK_KNN_HD bool hook_changes(int32_t old_parent, int32_t offered) { return old_parent > offered; }
// After a hook round on a flat forest that changed nothing, a cluster's root is its lowest core point; clusters are numbered by
// ascending root, which is the exclusive count of the roots below it.
SDFK_KNN_HD bool is_root(int32_t i, int32_t parent_i, bool core) { return core && parent_i == i; }
// the host's bound on the hook rounds: every round that changes something removes a tree
SDFK_KNN_HD int64_t max_rounds(int64_t n) { return n + 1; }

// ---- border ---------------------------------------------------------------------------------------------------------------------
// A point that is not core keeps the least key among the core candidates within the radius: the first in (d2, index) order, equal
// d2 to the lower index.  best starts at kKeyInf, which no candidate within a radius reaches.
SDFK_KNN_HD uint64_t border_take(uint64_t best, uint64_t key, uint64_t bound_key, bool candidate_is_core)
{
    return candidate_is_core && reaches(key, bound_key) && key < best ? key : best;
}
// the core point whose label the border point takes, -1: noise
SDFK_KNN_HD int32_t border_source(uint64_t best) { return best < kKeyInf ? sdfk_knn::key_index(best) : -1; }

// ---- select ---------------------------------------------------------------------------------------------------------------------
// any int32 per point selects: noise (-1), other negative labels and labels from n_clusters on are never kept (keep is not read)
SDFK_KNN_HD bool keeps(int32_t label, int64_t n_clusters, const uint8_t* keep) { return label >= 0 && (int64_t)label < n_clusters && keep[label] != 0; }

// ---- the argument checks: 0 accepted, else which refusal ----------------------------------------------------------------------------
enum { kArgsOk = 0, kArgsNullSet, kArgsRadius, kArgsMinPoints, kArgsNullLabels, kArgsClusterCount, kArgsNullKeep };
SDFK_KNN_HD int check_cluster_args(bool has_set, float radius, int32_t min_points)
{
    if (!has_set) return kArgsNullSet;
    if (!sdfk_knn::radius_is_valid(radius)) return kArgsRadius;   // (NaN and negative radii; +inf and 0 are accepted)
    if (min_points < 1) return kArgsMinPoints;
    return kArgsOk;
}
SDFK_KNN_HD int check_select_args(bool has_set, bool has_labels, bool has_keep, int64_t n_clusters)
{
    if (!has_set) return kArgsNullSet;
    if (!has_labels) return kArgsNullLabels;
    if (n_clusters < 0) return kArgsClusterCount;
    if (n_clusters > 0 && !has_keep) return kArgsNullKeep;
    return kArgsOk;
}

}  // namespace sdfk_cluster
