"""Sensitivity of the long-stream checks of test_gpu_streaming.py / test_gpu_stream_slots.py (no GPU): the float64 reverb
reference with one defect built in - the last 256-tap part never summed, the wet signal one sample late, reverb input lost or
stale once the ring has wrapped - must miss the 1e-4 bar those tests hold by a factor of ten or more, on the oracle's own dry
signal of the very inputs they stream."""
import pytest

from stream_long import F_LONG, conv64, defective_streams, long_inputs, oracle_reference, reverb_errors

BAR = 1e-4


@pytest.fixture(scope="module")
def reference(weights):
    from oracle.newt_oracle import OracleNEWT

    pre_ref, _ = oracle_reference(OracleNEWT(weights, fast=True, lut_python_loop=False), weights, *long_inputs(2))
    return pre_ref, weights["reverb.ir"][0]


def test_the_float64_reverb_passes_its_own_check(reference):
    pre, ir = reference
    full = conv64(pre, ir)
    N = 128 * F_LONG
    e = reverb_errors(pre + full[:, :N], pre, full[:, N:], ir)
    assert max(e.values()) <= 1e-12, e


DEFECTS = ["last_part_dropped", "one_sample_late", "input_lost_after_wrap", "stale_after_wrap"]


@pytest.fixture(scope="module")
def defect_errors(reference):
    pre, ir = reference
    return {name: reverb_errors(y, pre, tail, ir) for name, (y, tail) in defective_streams(pre, ir).items()}


@pytest.mark.parametrize("defect", DEFECTS)
def test_reverb_checks_trip_on_a_defect(defect_errors, defect):
    """RMS error each check sees (wet RMS 0.070; the bar is 1e-4):
                               whole     after_wrap   tail
        last_part_dropped      8.2e-4    1.04e-3      1.19e-3
        one_sample_late        1.22e-2   1.24e-2      3.97e-4
        input_lost_after_wrap  2.02e-2   6.89e-2      4.91e-3
        stale_after_wrap       2.54e-2   8.67e-2      8.00e-3
    Every defect misses at least one check by ten times the bar, and no check lets any of them through: the weakest pairs are
    the tail against a one-sample shift (4.0x: what still rings after the end is smooth) and the whole-run figure against the
    dropped part (8.2x: the 250 frames before that part reads anything dilute it; the figure over the last 48 frames does not)."""
    e = defect_errors[defect]
    print(defect, e)
    assert max(e.values()) >= 10 * BAR, e
    assert min(e.values()) >= 3 * BAR, e


@pytest.mark.parametrize("check", ["whole", "after_wrap", "tail"])
def test_every_reverb_check_has_a_defect_it_catches_tenfold(defect_errors, check):
    assert max(e[check] for e in defect_errors.values()) >= 10 * BAR
