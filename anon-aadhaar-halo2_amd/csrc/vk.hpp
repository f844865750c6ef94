// The verifying key (vk.hip makes, reads, writes and frees it; verify.hip verifies with it) and the view of a key that
// verify_core reads — what plonk::verify_proof [UP] takes from its VerifyingKey and its params: the circuit description,
// transcript_repr, omega, the fixed and permutation commitments and G = g[0].
#pragma once
#include <memory>
#include <vector>

#include "common.hpp"
#include "vkblob.hpp"

// Host data only: no device buffer, and no pointer to an amdzk_srs or an amdzk_pk (both may be gone when it is used).
struct amdzk_vk {
  std::shared_ptr<const pkblob::Desc> desc;  // shared with the proving key it was taken from, if any
  bn254::Fr transcript_repr, omega;
  std::vector<bn254::G1Affine> fixed_commitments, perm_commitments;
  bn254::G1Affine g;  // g[0] of the SRS the key was made on
};

// Exactly one of d_g (device; the proving key's route: g[0] where its SRS keeps it) and h_g (host; a verifying key's) is
// set, or neither for a proving key whose SRS has no monomial basis. Valid while the key it was built from lives.
struct zk_key_view {
  const pkblob::Desc* desc = nullptr;
  const bn254::Fr *transcript_repr = nullptr, *omega = nullptr;
  const bn254::G1Affine *fixed_commitments = nullptr, *perm_commitments = nullptr;
  const bn254::G1Affine *d_g = nullptr, *h_g = nullptr;
  const amdzk_pk* sized_by = nullptr;  // the proving key's route: amdzk_proof_size_multi must agree with the verifier's plan
};
