"""The LANCZOS_MODE_LSB1 contract, checked per sample (include/lanczos_hip.h) -- TEST INFRASTRUCTURE ONLY.

"Within 1 LSB" is what the mode promises callers; what the kernels actually do is tighter, and this checks that:
  * the H pass is bit-exact (f32 chains, the f64 chain for every sample within eps of an integer and for the integer-phase
    samples the flip filter cannot clear), so the V pass sees the reference's truncated intermediate T;
  * the V pass is an f32 chain with a host-proven error bound eps that stores floor(sum + eps) (k_march: eps - 0.5 and the RNE
    byte convert; k_fast / k_rat / k_ratp: the same convert or fmed3 + floor for 16-bit samples).  So a sample may differ from
    the reference only where the reference's own f64 sum v lies within 2 eps BELOW a store boundary, and then only upwards;
  * integer-phase rows >= K are copies of T's row in every fast family (k_march VPASS, k_fast VPASS, k_rat `rt.v_int`,
    k_ratp `r == 0`), so they equal T byte for byte;
  * rows < K come from the f64 prefix kernels (k_prefix_reg / k_prefix / k_prefix_stream / the RIDE workgroups), which recompute
    the rows they read from their own exact copy: they equal the reference;
  * k_generic is f64 throughout: bit-identical in every mode.
The per-sample work is oracle_explain_hwc_* (oracle/lanczos_oracle.c); |got - reference| <= 1 is asserted as well.

delta is the tolerance of the window (delta_for).  It must be at least 2 eps of every instance the library can launch:
tests/native/lsb1_eps_check.hip prints the eps of every instance against it and tests/test_lsb1_check.py asserts the result.
  * 8-bit samples: 2**-10 everywhere (the largest eps is 1.4e-4);
  * 16-bit samples: 2**-5, except where the library's proven bound is wider -- integer scales with a = 4 (eps 0.0175 from
    fast_prepare: 2 eps = 1.12 x 2**-5) take 2**-4, rational scales (k_rat / k_ratp: eps up to 0.036 at a = 4 from rat_prepare
    and ratp_prepare, whose bound prices the per-index weight deviations in full) take 2**-3.
Every one of these is far below what a precision regression costs (f16 weights: ~0.15 LSB at 8 bits, ~40 LSB at 16 bits) and
the check stays one-sided.
"""
import math

import numpy as np

import oracle_lib as O

DELTA_U8 = 2.0 ** -10
DELTA_U16 = 2.0 ** -5

# lanczos_hip.h LANCZOS_KERNEL_*
FAMILY_GENERIC = 1
FAMILY_FAST = 2

_KINDS = {1: "outside [store(v), store(v + delta)]", 2: "in-place prefix row (< K) differs from the reference",
          3: "integer-phase row is not a copy of the H intermediate's row"}


def delta_for(dtype, sn=1, sd=1, a=3):
    """The window of an instance; tests/native/lsb1_eps_check.hip uses the same rule (on the reduced scale)."""
    if np.dtype(dtype) == np.uint8:
        return DELTA_U8
    if sd // math.gcd(sn, sd) != 1:
        return 2.0 ** -3
    return 2.0 ** -4 if a == 4 else DELTA_U16


def check(img, sn, sd, a, got, family, what="", threads=16, delta=None):
    """Apply the LSB1 contract to one output `got` ([OUT_H][OUT_W][C]) of the request (img, sn/sd, a) served by kernel
    `family` (FAMILY_GENERIC: bit-identical; FAMILY_FAST: the checks above).  Fails with a readable message; returns the
    counts so that callers can assert coverage and report them."""
    img = np.ascontiguousarray(img)
    h, w, c = img.shape
    cfg = O.cfg(w, h, w * sn // sd, h * sn // sd, c, a, sn, sd)
    if family not in (FAMILY_GENERIC, FAMILY_FAST):
        raise AssertionError(f"{what}: kernel family {family} has no LSB1 contract here")
    d = delta_for(img.dtype, sn, sd, a) if delta is None else delta
    st, ref = O.explain_hwc(cfg, img, got, d, family == FAMILY_FAST, threads, want_ref=True)
    n_diff = max_diff = 0
    for r0 in range(0, got.shape[0], 256):          # (row blocks: full-size 16-bit frames stay small in memory)
        diff = np.abs(got[r0:r0 + 256].astype(np.int32) - ref[r0:r0 + 256].astype(np.int32))
        n_diff += int(np.count_nonzero(diff))
        max_diff = max(max_diff, int(diff.max()))
    assert max_diff <= 1, f"{what}: max |diff| {max_diff} > 1 LSB"
    if family == FAMILY_GENERIC:
        assert n_diff == 0, f"{what}: k_generic (f64 throughout) differs from the reference in {n_diff} samples"
    assert st.unexplained == 0, (
        f"{what}: {st.unexplained} of {st.samples} samples unexplained by the LSB1 contract (delta {d:g}, K = {st.inplace_rows}); "
        f"first at row {st.first_o}, column {st.first_x}, channel {st.first_c}: got {st.first_got}, reference f64 sum "
        f"v = {st.first_v!r} -- {_KINDS.get(st.first_kind, st.first_kind)}")
    return {
        "samples": int(st.samples), "equal": int(st.equal), "plus1": int(st.plus1), "window": int(st.window),
        "int_flips": int(st.int_flips), "int_row_samples": int(st.int_row_samples), "K": int(st.inplace_rows),
        "max_plus1_gap": float(st.max_plus1_gap), "plus1_fraction": st.plus1 / max(st.samples, 1), "delta": d,
    }


def explain(img, sn, sd, a, got, copies_int_rows=True, threads=8, delta=None):
    """The raw counts without asserting anything (the negative controls use it)."""
    img = np.ascontiguousarray(img)
    h, w, c = img.shape
    cfg = O.cfg(w, h, w * sn // sd, h * sn // sd, c, a, sn, sd)
    st, _ = O.explain_hwc(cfg, img, got, delta_for(img.dtype, sn, sd, a) if delta is None else delta, copies_int_rows, threads)
    return st
