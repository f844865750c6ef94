// workspace.hpp — who owns which scratch buffer of an amdzk_ctx, and the one way a reservation is cut into regions.
// Host-only and free of HIP, like witness.hpp, opening.hpp and verifier.hpp: a plain g++ program can include it
// (tests/native/workspace_check.cpp).
//
// THE RULES. A context (amdzk_ctx: the caller's, or one of its lanes, which is a context of its own with its own eight
// slots) holds ZK_WS_COUNT grow-only device buffers, handed out by zk_ws_reserve(ctx, slot, bytes, &p), and ONE grow-only
// pinned host buffer, handed out by zk_pinned_reserve.
//  * A reservation is a pointer, not a lock: the next reservation of the same slot on the same context gets the same
//    memory, or — when it asks for more — new memory. Growth waits for the context's stream before it frees, so a device
//    pointer from an earlier reservation stays good for the work already ENQUEUED with it, and is dead for the host: no
//    further copy, launch or read may be issued through it.
//  * Two users of one slot are therefore safe in exactly two cases:
//      (S) stream order: both only enqueue on the context's stream, and the first one's kernels have the region to
//          themselves until they have run, because the second one's come behind them;
//      (N) nesting: the outer user has enqueued its last access to its reservation before it calls the inner one, and does
//          not touch its own pointer afterwards.
//    Anything else — an outer user that still reads its region after an inner call reserved the slot — needs another slot.
//  * The pinned buffer has no stream order to lean on (the host reads it) and growth frees it at once: a pointer into it
//    is dead after ANY call that may reserve it again. Its users are zk_msm_finish (msm.hip), verify_core
//    (verify.hip), which has read everything it brought down before its first zk_msm_finish, and zk_pairing_products (pairing.hip),
//    which calls nothing between its reservation and its last read.
//  * A reservation promises the MEMORY, never its contents: a user that reserves a slot twice within one operation keeps
//    its first pointer (while nothing can have grown the slot) or writes everything again. What an earlier reservation
//    left is not there to be read, by the same user or another.
// The enum says for every shared slot which case holds and where.
//
// WHAT CHECKS THE RULES. AMDZK_WS_POISON=1, read once by amdzk_init (lanes follow their parent), fills scratch with the
// 32-bit word ZK_WS_POISON_WORD at the moment it is handed out:
//  * zk_ws_reserve fills the `bytes` it was asked for, on the context's stream: behind everything already enqueued, in
//    front of everything the new user enqueues. Correct code under (S) or (N) never sees it; an outer user that reads
//    its region after an inner reservation, a region read before it is written, or a call that counts on what the last
//    call left, reads the pattern and computes a wrong answer that a test against the reference sees;
//  * zk_pinned_reserve, and a proving key's staging ring when its bump pointer goes back to 0, fill the host memory at
//    once: a host pointer still read after a new reservation is caught too;
//  * zk_pk_poison (keygen.hip) fills the per-proof arenas of a key handle at the start of create_proof*, of the lock-step
//    batch and of amdzk_check_witness, and starts the handle's staging ring over; witness.hip and poseidon.hip fill their
//    handles' private buffers at the start of every run and every hash call.
//    THE LIMIT OF THE BATCH PATH: the lock-step batch fills every member's arenas once, in front of its first step, not
//    step by step. A step that reads what an EARLIER STEP OF THE SAME BATCH left in an arena is therefore not caught there;
//    the steps are the solo prover's (prove_steps), and it is caught through amdzk_create_proof* only as far as the solo
//    call shows the same dependence. What the batch path does catch: anything left by the call before.
// The word is 5 in every 32-bit word because a wrong read must give a wrong ANSWER, not a fault: as eight limbs it is a
// canonical non-zero Fr and Fq (top limb 5 < 0x30644e72), as an index, offset, count or loop bound it is small, as a
// flag it is set, as a point it is not on the curve. (0xFF bytes would be 4 billion as an index.)
// NOT POISONED, because no value is harmless as an address — regions whose content a kernel dereferences:
//    ZK_WS_TABLES (the whole slot); the reservations of ZK_WS_STAGING made with holds_addresses = true (the lock-step
//    batch's tables, Gang::scratch, and amdzk_msm_g1_cols_dev's column table); amdzk_pk::ptrs_l; amdzk_witness::d_ptrs.
//    A new reservation whose content is dereferenced passes holds_addresses = true to zk_ws_reserve.
// Nor is what a handle keeps from call to call scratch: of a key handle's arenas the first lk_const columns of ct hold the
// compressed constant lookup tables, written once at keygen (zk_pk_poison, keygen.hip, leaves them).
// With profiling on (amdzk_prof_enable) every fill counts as a launch of "ws_poison" in the profile map.
// A NEW DRIVER picks its slot by reading this file and is then run under the switch: tests/test_gpu_scratch_poison.py on
// a poisoned context of its own, or the whole suite with AMDZK_WS_POISON=1 in the environment (profiles/ws_poison_suite.txt).
// Every result must still equal the reference exactly. Off, the switch costs one host branch per reservation.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr uint32_t ZK_WS_POISON_WORD = 5;

enum ZkWs : int {
  // ntt.hip, zk_ntt_ex: the ping-pong buffer of a multi-pass transform. One user.
  ZK_WS_NTT = 0,
  // msm.hip: the counting sort, bucket lists and results of zk_msm_dev_xyzz, zk_msm_dev_xyzz_cols and
  // zk_msm_bases_dev_xyzz. (S) between MSMs — and the results live in the reservation: the caller brings them down
  // (zk_msm_finish) or copies them on the stream before it enqueues the next MSM on the same context.
  ZK_WS_MSM = 1,
  // Staging of the host-pointer entry points (capi.hip: amdzk_msm_g1_batch, _cols_dev, _bases_batch, amdzk_ntt_fr, _batch),
  // which return with the stream idle. Two more users:
  //  * the lock-step batch's pointer tables (prover.hip, Gang::scratch) — (S) among its own steps; no proof calls a
  //    host-pointer entry point, so the first group never runs inside it; the batch's phase callback
  //    (amdzk_batch_phase_fn) runs BETWEEN two steps, when the gang has enqueued its last access to the reservation, and
  //    what it may call — amdzk_witness_run keeps its scratch in its own handle — takes no slot of the ctx anyway;
  //  * srs_check_run (srs.hip) — it cannot use ZK_WS_STARTUP, its unit's slot: it still reads its column of combined
  //    points after zk_pairing_products has reserved that one. Nothing it calls touches this slot.
  ZK_WS_STAGING = 2,
  // The start-up calls: SRS setup, read, write, g_to_lagrange, downsize and the prefix-sum basis (srs.hip), (S) one behind
  // the other. Also verify_core (verify.hip) and zk_pairing_products (pairing.hip) — (N): the decide calls pair
  // after the core has returned, having read all it brought down, and no start-up call runs inside either.
  ZK_WS_STARTUP = 3,
  // zk_poly_eval, zk_lincomb, zk_kate_div (plonk_kernels.hip): partial sums that live for two launches. (S).
  ZK_WS_OPENING = 4,
  // amdzk_permute_expression_pair_dev (prover.hip). One user.
  ZK_WS_PERMUTE = 5,
  // Pointer and scalar tables that go up with a call: upload_ptrs_and_frs (plonk_kernels.hip), amdzk_multiopen_dev and
  // mo_verify_body (multiopen.hip). (S) between calls; amdzk_multiopen_dev hands zk_poly_eval, zk_lincomb and zk_kate_div
  // tables out of ITS reservation and never goes through upload_ptrs_and_frs.
  ZK_WS_TABLES = 6,
  // amdzk_batch_invert_dev, amdzk_batch_invert_assigned_dev, amdzk_grand_product_dev (plonk_kernels.hip). (S).
  ZK_WS_CALLS = 7,
  ZK_WS_COUNT = 8
};

// v rounded up to a multiple of a (a > 0). The one rounding function of the library's byte layouts and element counts.
constexpr size_t ws_round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The byte layout of one reservation: an offset counter. take() returns where the region starts and moves on to the next
// multiple of `pad` behind it; pad = 1 lets the next region follow without a gap. bytes(): the total so far.
struct WsLayout {
  size_t take(size_t bytes, size_t pad = 256) {
    const size_t at = off;
    off = ws_round_up(off + bytes, pad);
    return at;
  }
  size_t bytes() const { return off; }

 private:
  size_t off = 0;
};
