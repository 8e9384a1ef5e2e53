// Loader checks of zkmi_plonk_pk_set_commitments: what stands between a caller's commitment
// descriptors (gnark's api.Commit under PLONK, BSB22 [UPSTREAM-RECALL]; parity unpinned) and the
// kernels that use their words as row addresses.  Host-compilable, beside scs_check.h:
// tests/native/test_plonk_commit_check.cpp runs them without a GPU
// (tests/test_native_plonk_commit_check.py).
//
// Commitment i of a key on the domain of n = 2^log_n gate rows has its committed rows C_i (the
// selector Qcp_i is 1 there and 0 elsewhere), its commitment row r_i, and two blinding rows: r_i
// and the domain's last row n - 1, where pi2_i holds the caller's two blinding scalars.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

namespace zk {

constexpr uint32_t PLONK_MAX_COMMITMENTS = 8;   // ZKMI_PLONK_MAX_COMMITMENTS of include/zkmi.h

struct PlonkCommitShape {
  uint32_t n_rows;        // |C_i|
  const uint32_t* rows;   // C_i, host
  uint32_t row;           // r_i
  bool has_points;        // lag_g1 was given
  uint32_t lag_k;         // 0 = auto
};

// state of the key the descriptors are attached to
struct PlonkCommitKeyState {
  size_t n;               // rows of the domain
  bool attached;          // set_commitments has succeeded on this key before
  bool proved;            // a prove has started on this key
};

// "" when the whole set is accepted, else the reason; nothing is attached unless every one passes
inline std::string plonk_commit_validate(const PlonkCommitShape* c, uint32_t count,
                                         const PlonkCommitKeyState& key) {
  if (key.attached) return "plonk commitments: the key already carries its commitments";
  if (key.proved) return "plonk commitments: attach them before the key's first prove";
  if (count == 0 || !c) return "plonk commitments: nothing to attach";
  if (count > PLONK_MAX_COMMITMENTS)
    return "plonk commitments: " + std::to_string(count) + " commitments, at most " +
           std::to_string(PLONK_MAX_COMMITMENTS);
  const size_t last = key.n - 1;
  for (uint32_t i = 0; i < count; i++) {
    const std::string who = "plonk commitment " + std::to_string(i) + ": ";
    if (c[i].n_rows == 0 || !c[i].rows) return who + "no committed rows";
    if (!c[i].has_points) return who + "lag_g1 must not be null";
    if (c[i].lag_k != 0 && (c[i].lag_k < 4 || c[i].lag_k > 16))
      return who + "lag_k must be 0 or in [4,16]";
    if (c[i].n_rows > key.n) return who + "more committed rows than the domain has rows";
    if (c[i].row >= key.n)
      return who + "commitment row " + std::to_string(c[i].row) + " is outside the domain of " +
             std::to_string(key.n) + " rows";
    for (uint32_t j = 0; j < c[i].n_rows; j++) {
      const uint32_t r = c[i].rows[j];
      if (r >= key.n)
        return who + "committed row " + std::to_string(r) + " is outside the domain of " +
               std::to_string(key.n) + " rows";
      if (j && r <= c[i].rows[j - 1])
        return who + "committed rows must be ascending and unique (rows[" + std::to_string(j) +
               "] = " + std::to_string(r) + " after " + std::to_string(c[i].rows[j - 1]) + ")";
      if (r == c[i].row)
        return who + "its commitment row " + std::to_string(r) + " is one of its committed rows";
      if (r == last)
        return who + "Qcp is set at the blinding row " + std::to_string(r) +
               " (the last row of the domain)";
    }
  }
  return "";
}

// bases per subset-sum table of a commitment's n_rows + 2 Lagrange points (lag_k = 0)
inline uint32_t plonk_commit_auto_k(uint32_t n_points) { return n_points < 8 ? 4 : n_points < 64 ? 8 : 10; }

}  // namespace zk
