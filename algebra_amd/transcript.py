"""The Fiat-Shamir transcript of the device sumcheck -- the Python mirror of `Transcript` of
include/ark_hip.hpp and rust/ark-hip/src/sumcheck.rs.  The state is 32 bytes the caller initialises (a label, a statement
hash); `challenge(elements)` is one call of the host entry ark_hip_transcript_challenge:

    msg = state | u32_le(k) | le32(e_0) | .. | le32(e_{k-1});  out = SHAKE256(msg, 96);  state = out[:32];  c = out[32:] mod r

Elements go in and the challenge comes out as Montgomery uint64[4]; no device is needed.  The same operation runs inside the
kernels of `ListOfProducts.prove_device`, which advances a Transcript exactly as calling it once per round would."""
import ctypes as C

import numpy as np

from . import curves as cv
from ._lib import check, lib


class Transcript:
    def __init__(self, field, seed_bytes32):
        self.field = cv.field_id(field)
        seed = bytes(seed_bytes32)
        if len(seed) != 32:
            raise ValueError("the state is 32 bytes")
        self._state = (C.c_uint8 * 32)(*seed)

    @property
    def state(self):
        """the 32 bytes of state"""
        return bytes(self._state)

    def challenge(self, elements=None):
        """absorbs `elements` (uint64 [k, 4] Montgomery, k >= 0; None: none) and returns the challenge, uint64[4] Montgomery"""
        els = np.zeros((0, 4), dtype=np.uint64) if elements is None else np.ascontiguousarray(elements, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(4, dtype=np.uint64)
        check(lib().ark_hip_transcript_challenge(self.field, C.cast(self._state, C.c_void_p), els.ctypes.data_as(C.c_void_p) if len(els) else None,
                                                 len(els), out.ctypes.data_as(C.c_void_p)), "ark_hip_transcript_challenge")
        return out
