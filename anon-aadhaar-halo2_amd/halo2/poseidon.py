"""Poseidon over Fr on the device (include/amdzk.h "Poseidon over Fr"): batched permutations and sponges.

A Spec carries the textbook round constants and the MDS matrix as integers — the library generates none; what it computes
for them is stated in the header. Poseidon(ctx, spec) compiles it for ctx's device: update / squeeze hash one sponge with the
`poseidon` crate's names (parity unpinned), hash_many and permute_many serve batches over numpy arrays and device buffers."""
import ctypes as C

import numpy as np

from .. import ffi as _ffi

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def mont_words(v):
    """The 4 x u64 Montgomery words of the integer v mod r."""
    v = (v % R) * (1 << 256) % R
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def to_fr(values):
    """Integers -> (n, 4) uint64 Montgomery words."""
    return np.array([mont_words(v) for v in values], dtype=np.uint64).reshape(-1, 4)


def from_fr(words):
    """(n, 4) uint64 Montgomery words -> integers."""
    rinv = pow(1 << 256, -1, R)
    return [sum(int(w) << (64 * i) for i, w in enumerate(row)) * rinv % R for row in np.asarray(words, dtype=np.uint64).reshape(-1, 4)]


class Spec:
    """t, rate, r_f, r_p; round_constants: (r_f + r_p) rows of t integers; mds: t rows of t integers; initial_state: t
    integers, or None for (2^64, 0, ..., 0)."""

    def __init__(self, t, rate, r_f, r_p, round_constants, mds, initial_state=None):
        self.t, self.rate, self.r_f, self.r_p = t, rate, r_f, r_p
        self.round_constants = [list(row) for row in round_constants]
        self.mds = [list(row) for row in mds]
        self.initial_state = None if initial_state is None else list(initial_state)

    def desc(self, size=None):
        """(amdzk_poseidon_desc, keep-alive list). The integers are reduced mod r."""
        rc = to_fr([v for row in self.round_constants for v in row])
        mds = to_fr([v for row in self.mds for v in row])
        init = None if self.initial_state is None else to_fr(self.initial_state)
        d = _ffi.PoseidonDesc(C.sizeof(_ffi.PoseidonDesc) if size is None else size, self.t, self.rate, self.r_f, self.r_p, rc.ctypes.data,
                              mds.ctypes.data, None if init is None else init.ctypes.data)
        return d, [rc, mds, init]

    def check(self):
        """amdzk_poseidon_check_desc (no device needed): raises AmdzkError with the refusal's message."""
        d, keep = self.desc()
        check_desc(d)
        del keep


def check_desc(d):
    msg = C.create_string_buffer(256)
    rc = _ffi.lib().amdzk_poseidon_check_desc(C.byref(d) if d is not None else None, msg, len(msg))
    if rc != 0:
        raise _ffi.AmdzkError(rc, msg.value.decode())


class Poseidon:
    """amdzk_poseidon: the spec resident on ctx's device. One call at a time."""

    def __init__(self, ctx, spec):
        self.ctx, self.t, self.rate = ctx, spec.t, spec.rate
        d, keep = spec.desc()
        h = C.c_void_p()
        ctx._chk(ctx.L.amdzk_poseidon_compile(ctx.h, C.byref(d), C.byref(h)))
        del keep
        self.h = h
        self._buf = []

    # ---- one sponge, with the crate's names: update takes integers, squeeze returns one
    def update(self, values):
        self._buf.extend(int(v) % R for v in values)
        return self

    def squeeze(self):
        """The digest of everything updated so far; the sponge starts afresh."""
        out = self.hash_many([to_fr(self._buf)])
        self._buf = []
        return from_fr(out)[0]

    # ---- batches
    def hash_many(self, inputs):
        """amdzk_poseidon_hash. inputs: one (len_b, 4) uint64 array of Montgomery words per sponge (or an (n, len, 4) array).
        Returns the digests, (n, 4) uint64."""
        rows = [np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4) for x in inputs]
        n = len(rows)
        ptrs = (C.c_void_p * max(1, n))(*[r.ctypes.data if r.size else None for r in rows])
        lens = (C.c_size_t * max(1, n))(*[r.shape[0] for r in rows])
        out = np.zeros((n, 4), dtype=np.uint64)
        self.ctx._chk(self.ctx.L.amdzk_poseidon_hash(self.ctx.h, self.h, ptrs, lens, n, out.ctypes.data))
        return out

    def hash_many_dev(self, d_inputs, input_stride, n, d_out, out_stride=1, lens=None, length=0, in_offset=0, out_offset=0):
        """amdzk_poseidon_hash_dev: input a of sponge b at d_inputs + in_offset + b * input_stride + a (in Fr), digest b to
        d_out + out_offset + b * out_stride. lens: n lengths, or None for "all `length`"."""
        lens_c = None if lens is None else (C.c_size_t * max(1, len(lens)))(*lens)
        assert lens is None or len(lens) == n
        self.ctx._chk(self.ctx.L.amdzk_poseidon_hash_dev(self.ctx.h, self.h, _at(d_inputs, in_offset), input_stride, lens_c, length, n,
                                                         _at(d_out, out_offset), out_stride))

    def permute_many_dev(self, d_states, n_states, state_stride=None, offset=0):
        """amdzk_poseidon_permute_dev: state b at d_states + offset + b * state_stride (in Fr), permuted in place."""
        self.ctx._chk(self.ctx.L.amdzk_poseidon_permute_dev(self.ctx.h, self.h, _at(d_states, offset), n_states,
                                                            self.t if state_stride is None else state_stride))

    def permute_many(self, states):
        """(n, t, 4) uint64 Montgomery words -> the permuted states, through a device buffer of their size."""
        states = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, self.t, 4)
        d = self.ctx.alloc(max(states.nbytes, 32))
        try:
            d.upload(states)
            self.permute_many_dev(d, states.shape[0])
            return d.download(states.shape)
        finally:
            d.free()

    def free(self):
        if self.h:
            self.ctx.L.amdzk_poseidon_free(self.ctx.h, self.h)
            self.h = None


def _at(dbuf, offset_fr):
    """A DeviceBuffer (or None, or a raw address) advanced by offset_fr field elements."""
    if dbuf is None:
        return None
    base = dbuf.ptr.value if hasattr(dbuf, "ptr") else int(dbuf)
    return C.c_void_p(base + 32 * offset_fr)
