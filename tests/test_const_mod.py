"""The compile-time modulus constants of the constant-modulus kernels (csrc/hip/dev.h ModK<q>) against the ModC
table the run-time forms use (csrc/hip/host_util.h make_modc), for every odd prime up to 37, and both against the
formulas written out here. Host arithmetic only: no device is needed.

The kernels dispatch on the odd primes up to 17 (dev.h modk_dispatch); the evaluator repeats this comparison for
those when it uploads its ModC table (hostutil::modk_table_ok)."""
import pytest

PRIMES = [3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37]
FIELDS = ("q", "n", "c", "D", "Dn", "v", "sh")


def _by_hand(q):
    n = 0
    while q ** (n + 1) < 1 << 128:  # core.h nr_comps: floor(128 / log2 q)
        n += 1
    c = 1
    while q ** (c + 1) <= 1 << 31:  # the longest chunk with D = q^c <= 2^31
        c += 1
    D = q ** c
    sh = 32 - D.bit_length()
    Dn = D << sh
    v = ((1 << 64) - 1) // Dn - (1 << 32)  # Moller-Granlund reciprocal of the normalised divisor
    return (q, n, c, D, Dn, v, sh)


@pytest.mark.parametrize("q", PRIMES)
def test_modk_equals_modc(native, q):
    nat = native
    k, m = nat.hip_modk_constants(q), nat.hip_modc_constants(q)
    assert k is not None
    assert dict(zip(FIELDS, k)) == dict(zip(FIELDS, m))
    assert tuple(int(x) for x in k) == _by_hand(q)
    assert k[1] == nat.nr_comps(q)


def test_no_constant_form_elsewhere(native):
    nat = native
    for q in (2, 4, 9, 15, 41, 256):
        assert nat.hip_modk_constants(q) is None


def test_chain_rule(native):
    nat = native
    assert nat.hip_chain_const_mod_pick([2, 3, 5, 7, 11, 13, 17])
    assert not nat.hip_chain_const_mod_pick([2, 3, 5, 7, 11, 13, 19])  # seven residues, not the first primes
    assert not nat.hip_chain_const_mod_pick([2, 3, 5, 7, 11, 13])      # first primes of another K
    assert not nat.hip_chain_const_mod_pick([2, 3, 5, 7, 11, 13, 17, 19])
