"""GPU suite: mi_scan_context_search on the cases of tests/scan_context_scale_cases.py, against S.search_pruned bit for bit through
check_search of tests/test_gpu_scan_context.py, without a tolerance anywhere, and mi_scan_context on a batch of 300 scans.  What the cases
reach that the first suite does not: chunks of several 64-row units, so a wave's row loop across unit boundaries with the next row's
operand prefetched across them; a last chunk and a last unit that are partial; limits that end inside a long chunk and limits that cut
whole chunks off; a runner-up pass whose winner lies in another chunk, or with the other wave, than the runner-up; rows at and above 2^16
and 2^20 in the packed key and out of it again.  tests/test_scan_context_scale_cases.py shows on the CPU that the restatement equals the
full one wherever that is affordable, and which plan every case takes at 32, 64, 256 and 304 CUs; each test here prints the device's CU
count and the plan it took."""
import ctypes as C

import numpy as np
import pytest

import scan_context_reference as S
import scan_context_scale_cases as K
from test_gpu_scan_context import check_search, same, shape_params

pytestmark = pytest.mark.gpu

HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT = 63       # hipDeviceAttribute_t (hip_runtime_api.h)


def cu_count(capi):
    """multiProcessorCount of device 0, which the context of the session is on and sizes its chunks by.  The library does not report it;
    the HIP runtime it is linked to does, and a symbol of a library's dependencies resolves through the library's handle."""
    n = C.c_int(0)
    f = capi.lib().hipDeviceGetAttribute
    f.argtypes, f.restype = [C.POINTER(C.c_int), C.c_int, C.c_int], C.c_int
    assert f(C.byref(n), HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT, 0) == 0 and 0 < n.value <= 4096, n.value
    return n.value


def searched(ctx, capi, name):
    c, want = K.CASES[name](), K.reference(name)
    nq, nd = len(c["query"]), len(c["db"])
    cus = cu_count(capi)
    print("%s: %d CUs, nq %d, nd %d: chunk_len %d, %d chunks, the last of %d rows" % ((name, cus, nq, nd) + K.plan(nq, nd, cus)))
    params, _ = shape_params(capi, c["rings"], c["sectors"])
    got = check_search(ctx, params, c["query"], c["db"], limit=c["limit"], label=name, want=want)      # with and without the runner-up
    again = ctx.scan_context_search(c["query"], c["db"], limit=c["limit"], params=params, want_second=True)
    assert all(same(a, b) for a, b in zip(again, got)), name                                            # the same call, the same bits
    return c, got


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_search(ctx, capi, name):
    c, (idx, dist, shift, second) = searched(ctx, capi, name)
    if c["limit"] is not None:
        seen = c["limit"] > 0
        assert seen.any() and (idx[seen] >= 0).all() and (idx[seen] < c["limit"][seen]).all() and (idx[~seen] == -1).all()
    if name == "high_rows":
        assert idx.tolist() == list(K.HIGH_PLANTED)


def test_a_batch_of_300_scans(ctx, capi):
    params, tables = shape_params(capi, 20, 60)
    clouds, centres = K.batch()
    batch = ctx.scan_context(list(clouds), centres=centres, params=params)
    assert batch.shape == (K.BATCH_SCANS, 20, 60) and same(batch, S.descriptors(clouds, centres, params, tables))
    assert (batch > 0).any(axis=(1, 2)).sum() > 150
    for i in K.BATCH_SAMPLED:                                            # a scan's descriptor does not depend on the batch
        assert same(ctx.scan_context([clouds[i]], centres=centres[i:i + 1], params=params)[0], batch[i]), i
    assert same(ctx.scan_context(list(clouds), centres=centres, params=params), batch)


def test_more_rows_than_the_key_holds_are_refused_before_anything_is_read(ctx, capi):
    params = capi.scan_context_params(rings=7, sectors=13)
    query, db = K.near_ties_7x13()["query"][:5], K.near_ties_7x13()["db"]                        # 100 rows: nothing behind them may be read
    outs = dict(idx=np.full(5, -7, np.int32), dist=np.full(5, -7.5, np.float32), shift=np.full(5, -7, np.int32), second=np.full(5, -7.5, np.float32))
    limit = np.full(5, 100, np.int32)
    max_rows = 1 << 26                                                   # MI_SCAN_CONTEXT_MAX_ROWS (tests/test_scan_context_abi.py)
    for lim in (None, limit):
        rc = capi.scan_context_search_raw(ctx._h, query.ctypes.data, 5, db.ctypes.data, max_rows + 1, None if lim is None else lim.ctypes.data,
                                          C.addressof(params), outs["idx"].ctypes.data, outs["dist"].ctypes.data, outs["shift"].ctypes.data,
                                          outs["second"].ctypes.data)
        msg = capi.lib().mi_last_error().decode()
        assert rc == capi.MI_ERR_INVALID_ARG and msg.startswith("mi_scan_context_search:") and "more than" in msg, msg
        assert (outs["idx"] == -7).all() and (outs["dist"] == -7.5).all() and (outs["shift"] == -7).all() and (outs["second"] == -7.5).all()
    want = K.reference("near_ties_7x13")                                 # the context is as usable as before
    got = ctx.scan_context_search(query, db, params=params, want_second=True)
    assert all(same(a, b[:5]) for a, b in zip(got, want))
