"""Which kernel a call launched, read from the library's launch profiler (shared by the conv unit tests)."""


def launches_of(rt, call, level=1):
    """Runs call() with the launch profiler on (dtts_profile_enable(1) resets the totals; the profiler is process-wide) and returns
    (call's result, {kernel tag: launches}) of every MFMA kernel the call launched, e.g. {"conv_gemm_kernel<64,64,k16>": 1}.
    level = 2: the bandwidth-only helper kernels (GroupNorm / split passes) are counted too."""
    rt.profile_enable(level)
    try:
        out = call()
        report = rt.profile_report()
    finally:
        rt.profile_enable(False)
    return out, {e["name"]: e["launches"] for e in report}
