"""Which kernel family a test's products really run on: every ops.gemm / ops.gemm_raw call inside `recorded()` first asks ops.gemm_plan (pero_gemm_plan:
the decision pero_gemm itself launches from) with the same arguments and under the options in force at that moment."""
import contextlib


@contextlib.contextmanager
def recorded():
    """Yields the list of the families ("t128", "r256", "e256", ...) of the products issued inside the block, in call order."""
    from pero_pretraining_amd import ops
    log = []
    raw = ops.gemm_raw

    def spy(*args, **kw):
        log.append(ops.gemm_plan(*args, **kw)[0])
        return raw(*args, **kw)

    ops.gemm_raw = spy
    try:
        yield log
    finally:
        ops.gemm_raw = raw
