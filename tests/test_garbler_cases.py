"""The garbler edge cases (tests/garbler_cases.py) on the host: every case garbles, evaluates to the plaintext
quantized result and garbles deterministically, so the reference side of the GPU comparisons in
tests/test_gpu_garbler_forms.py is sound on a machine without a GPU."""
import numpy as np
import pytest

from dash_amd.garbling import GarbledCircuit
from tests import garbler_cases as gcs

SEED = bytes(range(16))
CASES = gcs.all_cases()


def test_case_list_shape():
    names = [c.name for c in CASES]
    assert len(names) == len(set(names))
    kinds = {c.kind for c in CASES}
    assert {"sign", "relu", "rescale_legacy", "rescale_mrs", "relu_mrs", "joint", "redash", "base_ext", "maxpool2",
            "maxpool3", "max", "sumpool_relu", "dense", "dense_tf"} <= kinds
    for kind in ("sign", "relu_mrs", "joint", "redash", "maxpool3", "dense"):
        assert {c.N for c in CASES if c.kind == kind} >= set(gcs.SIZES), kind
    assert [32, 167, 173] in [c.bases()[0] for c in CASES]
    assert {len(c.bases()[0]) for c in CASES} >= {2, 3, 9}
    assert {c.name for c in gcs.child_cases()} == {
        "sign-hard-n65", "sign-ref-n65", "rescale_mrs-hard-n65", "joint-hard-n65", "redash-hard-n65", "redash-ref-n65",
        "maxpool3-hard-n65", "maxpool3-ref-n65"}


def test_pool_geometries_hit_the_sizes():
    for N in gcs.SIZES:
        for k, (C, H, W) in ((2, gcs.POOL2[N]), (3, gcs.POOL3[N])):
            assert H % k == 0 and W % k == 0 and C * (H // k) * (W // k) == N
        assert gcs.MAXN[N] // 2 == N and gcs.DENSE[N][1] == N


@pytest.mark.parametrize("q", list(range(2, 256)) + [256, 257, 1024, 4093, 4096])
def test_compress_class_restatement(native, q):
    """The Python restatement the GPU coverage assertion uses == the predicate the kernels dispatch on."""
    assert gcs.compress_class(q) == native.hip_garbler_compress_class(q)


def test_approx_sign_needs_an_mrs_base():
    """The finding behind the k = 2 / k = 3 cases: without an MRS base the approximate sign is refused."""
    import dash_amd as d

    with pytest.raises(RuntimeError, match="non-empty MRS base"):
        GarbledCircuit(d.Circuit([d.Sign((3,))]), 3, None, seed=SEED)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_on_host(case):
    c, crt, mrs, kw = case.build()
    a = GarbledCircuit(c, crt, mrs, seed=SEED, **kw)
    assert a.hardened == case.hardened
    x = case.inputs()
    y = a.decode_outputs(a.cpu_evaluate(a.garble_inputs(x)))
    np.testing.assert_array_equal(y, a.plain_q_eval(x))
    c2, crt2, mrs2, kw2 = case.build()
    b = GarbledCircuit(c2, crt2, mrs2, seed=SEED, **kw2)
    assert gcs.digest(a) == gcs.digest(b)


def test_parse_log():
    recs = gcs.parse_log(["entry sign N=65 k=7", "launch k_bank grid=3 blocks=9 cap=32768",
                          "project keys=iu hard=1 by_i=1 N=65 scopes=2 tsh=3,5 emit_blocks=12 lds=100 bank_paired=1 "
                          "bank_single=0 hash=k_hash_iu<16,hard> xa=2:g8,167:rt3"])
    assert recs[0] == {"what": "entry", "name": "sign", "N": 65, "k": 7}
    assert recs[1]["grid"] == 3 and recs[1]["blocks"] == 9
    assert recs[2]["tsh"] == [3, 5] and recs[2]["xa"] == {2: "g8", 167: "rt3"} and recs[2]["keys"] == "iu"
