// points_orient.h -- the decisions of the consistent orientation of point-cloud normals (lib_orient.hip), written once for the
// device and the host: which normals take part, the dot of two normals, the order in which seeds are taken and their sign, and
// the choice one point makes from its row of neighbours in one round.  Plain C++ outside hipcc, so that
// tests/cpp/points_orient_host.cpp checks it as the kernels run it; tests/orient_model.py restates it in numpy.
// Contract: include/sdfkit_hip.h, "Point clouds: a consistent orientation".
//
// Binary64 from the f32 inputs, one rounding per written operation, in the order written (-ffp-contract=off); the products of two
// widened f32 are exact.
#pragma once
#include "points_knn.h"

#define SDFK_OR_HD SDFK_KNN_HD

namespace sdfk_orient {

constexpr int kMinK = 2;
constexpr int kLevels = 4;
// the least weight |dot| an edge needs at each level: confident edges first.  All exact in binary64.
SDFK_OR_HD double threshold(int level) { return level == 0 ? 0.9375 : level == 1 ? 0.75 : level == 2 ? 0.5 : 0.0; }

// A normal takes part iff its components are finite and not all zero (either sign of zero).
SDFK_OR_HD bool valid(const float n[3])
{
    for (int a = 0; a < 3; a++)
        if ((sdfk_knn::f32_bits(n[a]) & 0x7f800000u) == 0x7f800000u) return false;   // NaN or +-inf
    return !(n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f);
}

SDFK_OR_HD double dot(const float a[3], const float b[3])
{
    return ((double)a[0] * (double)b[0] + (double)a[1] * (double)b[1]) + (double)a[2] * (double)b[2];
}

// ---- seeds ---------------------------------------------------------------------------------------------------------------------
// The next seed is the unoriented valid point of greatest p_z (f32 compare: -0 equals +0, a NaN counts as -inf), ties to the
// lowest index.  As one integer: the greatest key (order-preserving bits of z) << 32 | (2^32 - 1 - index); 0 means no point.
SDFK_OR_HD uint64_t seed_key(float z, int32_t index)
{
    if (!(z == z)) z = -INFINITY;
    if (z == 0.0f) z = 0.0f;   // -0 -> +0
    const uint32_t b = sdfk_knn::f32_bits(z);
    const uint32_t ordered = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return (uint64_t)ordered << 32 | (0xffffffffu - (uint32_t)index);
}
SDFK_OR_HD int32_t seed_index(uint64_t key) { return (int32_t)(0xffffffffu - (uint32_t)key); }

// The sign (+1 keep, -1 flip) that makes a seed's n_z positive; n_z == 0: the component of largest magnitude positive, ties to
// the lowest axis (sdfk_points_normals' rule without a viewpoint).
SDFK_OR_HD int seed_sign(const float n[3])
{
    if (n[2] > 0.0f) return 1;
    if (n[2] < 0.0f) return -1;
    float big = n[0], mag = n[0] < 0.0f ? -n[0] : n[0];
    const float m1 = n[1] < 0.0f ? -n[1] : n[1];
    if (m1 > mag) { mag = m1; big = n[1]; }
    return big < 0.0f ? -1 : 1;   // (n_z == 0 has magnitude 0: it never wins, and cannot tie a valid normal's largest)
}

// ---- one point's choice in a round ------------------------------------------------------------------------------------------------
// A row entry j is a source in round r iff its normal is valid and it was oriented in an earlier round: 0 < stamp_j < r.
SDFK_OR_HD bool is_source(int32_t stamp, int32_t round, const float n[3]) { return stamp > 0 && stamp < round && valid(n); }

// The sources of a row are offered in row order; the one of greatest |dot| stays, ties to the first.
struct Choice {
    bool any = false;
    double weight = 0.0, signed_dot = 0.0;   // |dot(i, j)| and dot(i, j) * s_j of the source kept
    SDFK_OR_HD void offer(const float ni[3], const float nj[3], int sj)
    {
        const double d = dot(ni, nj);
        const double w = d < 0.0 ? -d : d;
        if (!any || w > weight) {
            any = true;
            weight = w;
            signed_dot = d * (double)sj;
        }
    }
    SDFK_OR_HD bool accepted(int level) const { return any && weight >= threshold(level); }
    SDFK_OR_HD int sign() const { return signed_dot < 0.0 ? -1 : 1; }   // (a dot of exactly 0 says nothing: the normal is kept)
};

// the level of the round after one at `level` that oriented `count` points; kLevels: the growth of this seed is over
SDFK_OR_HD int next_level(int level, unsigned count) { return level >= kLevels ? kLevels : level + (count == 0u ? 1 : 0); }

// the output: the sign bit of every component flipped
SDFK_OR_HD float flipped(float x) { return sdfk_knn::bits_f32(sdfk_knn::f32_bits(x) ^ 0x80000000u); }

}  // namespace sdfk_orient
