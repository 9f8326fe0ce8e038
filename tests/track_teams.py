"""The closed loops' team sizes, restated in Python: csrc/launch_plan.h gc_block_lowrate_level and csrc/track_plan.h's team
formulae (gc_plan_track_device, gc_plan_track_host).  tests/test_track_plan_cpu.py holds the planners against them without a GPU,
tests/test_gpu_loop_epochs.py holds gc_debug_last_track_team against them on the device.  `S`: a settings object (samplingFreq,
codeFreqBasis, codeLength)."""


def _lowrate(step):
    return 2 if 15.0 * step < 0.995 else 1 if 7.0 * step < 0.995 else 0


def _fast_device_team(cu, nch, S, i8c=True):
    lr = _lowrate(S.codeFreqBasis * 1.001 / S.samplingFreq)
    assert lr > 0, "not a rate the fast kernel accepts"
    spl = 16 if (lr == 2 and i8c) else 8
    chunks = int(S.codeLength / (S.codeFreqBasis / S.samplingFreq) / spl) + 1
    return max(1, min(32, (4 * cu + nch - 1) // nch, max(1, chunks // 32)))


def _fast_host_team(cu, nch, S):
    lr = _lowrate(S.codeFreqBasis * 1.001 / S.samplingFreq)
    assert lr > 0, "not a rate the fast kernel accepts"
    approx_chunks = int(S.codeLength / (S.codeFreqBasis / S.samplingFreq) / 8.0) + 1
    return max(1, min(32, (4 * cu + nch - 1) // nch, max(1, approx_chunks * 8 // (16 if lr == 2 else 8) // 48)))


def _lane_device_team(cu, nch, arms, blksize):
    return max(1, min({1: 8, 2: 6}[arms], blksize // (64 * 8 * 2), max(1, 2 * cu // nch)))


def _halvings(team):
    """A team and what gc_track / gc_track_device make of it while the persistent grid is not resident whole: halved until it fits."""
    chain = [team]
    while chain[-1] > 1:
        chain.append((chain[-1] + 1) // 2)
    return chain
