"""The model of the library's Fiat-Shamir transcript, from hashlib.shake_256 and Python integers:

    msg = state | u32_le(k) | le32(e_0) | .. | le32(e_{k-1});  out = SHAKE256(msg, 96);  state = out[:32];  c = int_le(out[32:]) mod r

on CANONICAL values, and a driver that runs the round model and the verifier of tests/sumcheck_ref.py with challenges from it."""
import hashlib

import pyref
import sumcheck_ref as S


class Transcript:
    def __init__(self, p, seed):
        assert len(seed) == 32
        self.p, self.state = p, bytes(seed)

    def challenge(self, elements=()):
        """canonical integers in, the canonical challenge out"""
        msg = self.state + len(elements).to_bytes(4, "little") + b"".join((e % self.p).to_bytes(32, "little") for e in elements)
        out = hashlib.shake_256(msg).digest(96)
        self.state = out[:32]
        return int.from_bytes(out[32:], "little") % self.p

    def copy(self):
        return Transcript(self.p, self.state)


def reduce512(bytes64, p):
    """int_le(64 bytes) mod p as the Montgomery limbs (uint64[4]) the library returns"""
    return pyref.to_mont(int.from_bytes(bytes64, "little") % p, p)


def prove(tables, terms, transcript, p):
    """sumcheck_ref.prove with the challenge after round i = transcript.challenge(evals_i); advances the transcript"""
    return S.prove(tables, terms, lambda i, g: transcript.challenge(g), p)


def verify(claim, rounds, point, finals, terms, transcript, p):
    """The verifier with its own copy of the transcript: the point must be the challenges the transcript gives for the
    rounds, and sumcheck_ref.verify must accept.  Advances the transcript."""
    for g, r in zip(rounds, point):
        if transcript.challenge(g) != r:
            return False
    return S.verify(claim, rounds, point, finals, terms, p)
