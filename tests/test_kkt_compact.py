"""CPU-side checks of the compact (structure-aware) block entry points: widths, coverage and
argument validation are host logic -- no launch, no GPU (the library loads without a device)."""
import ctypes


def _fams():
    from noc import problems
    return (problems.cartpole(0.005).family.to_c(), problems.pendulum(0.01).family.to_c(),
            problems.double_integrators(4, 0.001).family.to_c(),
            problems.double_integrators(1, 0.1).family.to_c())


def test_compact_widths():
    from noc import _lib
    lib = _lib.load()
    cart, pend, lin8, lin2 = _fams()
    fields = (_lib.FIELD_A, _lib.FIELD_B, _lib.FIELD_Q, _lib.FIELD_R, _lib.FIELD_M)
    assert [lib.noc_compact_width(ctypes.byref(cart), f) for f in fields] == [4, 2, 3, 1, 1]
    assert sum(lib.noc_compact_width(ctypes.byref(pend), f) for f in fields) == 3
    assert lib.noc_compact_width(ctypes.byref(cart), 5) == -1
    assert lib.noc_compact_width(ctypes.byref(cart), -1) == -1
    assert lib.noc_compact_width(ctypes.byref(lin8), _lib.FIELD_A) == -1
    assert lib.noc_compact_width(None, _lib.FIELD_A) == -1


def test_compact_coverage():
    from noc import _lib
    lib = _lib.load()
    cart, pend, lin8, lin2 = _fams()
    for fam in (cart, pend):
        for lanes in (8, 16, 32, 64):
            assert lib.noc_kkt_compact_supported(ctypes.byref(fam), 200, lanes) == 1
        for lanes in (128, 1, 0, 48):
            assert lib.noc_kkt_compact_supported(ctypes.byref(fam), 200, lanes) == 0
        assert lib.noc_kkt_compact_supported(ctypes.byref(fam), 0, 32) == 0
    for fam in (lin8, lin2):
        assert lib.noc_kkt_compact_supported(ctypes.byref(fam), 200, 32) == 0
    assert lib.noc_kkt_compact_supported(None, 200, 32) == 0
    bad = _fams()[0]
    bad.nx = 3
    assert lib.noc_kkt_compact_supported(ctypes.byref(bad), 200, 32) == 0


def test_compact_entry_points_reject_bad_arguments_before_any_launch():
    from noc import _lib
    lib = _lib.load()
    cart, pend, lin8, lin2 = _fams()
    p = 16  # a 16-byte aligned fake device address: never dereferenced
    blocks, outs = [p] * 7, [p, p, p, p, p, p, None, None]

    def solve(fam=cart, N=10, B=4, lanes=32, blocks=blocks):
        return lib.noc_kkt_solve_compact(ctypes.byref(fam) if fam is not None else None, N, B, lanes,
                                         *blocks, None, None, None, *outs, None)
    assert solve(B=0) == 0                      # an empty batch validates and returns
    assert solve(fam=None) == -1
    assert solve(fam=lin8) == -1 and b"compact" in lib.noc_last_error()
    assert solve(lanes=128) == -1 and b"lanes" in lib.noc_last_error()
    assert solve(lanes=1) == -1
    assert solve(N=0) == -1 and b"horizon" in lib.noc_last_error()
    assert solve(B=-1) == -1
    for i in range(7):                          # A, B, Q, R, M, r, P are required
        assert solve(blocks=blocks[:i] + [None] + blocks[i + 1:]) == -1
        assert b"NULL" in lib.noc_last_error()
    assert solve(blocks=[24] + blocks[1:]) == -1 and b"aligned" in lib.noc_last_error()
    # K = d = NULL where the gains do not fit on chip
    rc = lib.noc_kkt_solve_compact(ctypes.byref(cart), 2000, 4, 32, *blocks, None, None, None,
                                   p, p, p, p, None, None, None, None, None)
    assert rc == -1 and b"noc_kkt_gains_on_chip" in lib.noc_last_error()

    def expand(fam=cart, N=10, B=4, lanes=32, ptrs=[p] * 10):
        return lib.noc_blocks_expand(ctypes.byref(fam) if fam is not None else None, N, B, lanes,
                                     *ptrs, None)
    assert expand(B=0) == 0
    assert expand(fam=None) == -1
    assert expand(fam=lin2) == -1
    assert expand(lanes=128) == -1
    assert expand(N=0) == -1
    for i in range(10):
        assert expand(ptrs=[p] * i + [None] + [p] * (9 - i)) == -1

    ws = _lib.NocIpmWs()
    ws.Bt, ws.N, ws.lanes = 4, 50, 32
    for f in _lib.WS_DOUBLE_FIELDS + _lib.WS_INT_FIELDS + _lib.WS_STATE_FIELDS:
        setattr(ws, f, 16)
    w = ctypes.byref(ws)
    twins = (lambda f, w: lib.noc_ipm_prepare_compact(f, w, 0, 0, None),
             lambda f, w: lib.noc_ipm_step_compact(f, w, 0, 0, 0, None),
             lambda f, w: lib.noc_ipm_step_main_compact(f, w, 0, 0, None))
    for call in twins:
        assert call(None, w) == -1
        assert call(ctypes.byref(cart), None) == -1
        assert call(ctypes.byref(lin2), w) == -1 and b"compact" in lib.noc_last_error()
    ws.lanes = 1
    for call in twins:
        assert call(ctypes.byref(cart), w) == -1
    ws.lanes, ws.flags = 32, 8                  # no new flags bit: bit 8 stays rejected
    for call in twins:
        assert call(ctypes.byref(cart), w) == -1 and b"flags" in lib.noc_last_error()
    ws.flags, ws.Bt = 0, 0                      # an empty workspace validates and returns
    for call in twins:
        assert call(ctypes.byref(cart), w) == 0
    assert lib.noc_ipm_step_compact(ctypes.byref(cart), w, 0, 0, 64, None) == -1  # lanes != ws->lanes
