"""The three kernels that turn a packed state into network input -- k_leaf_stem (tables by k_stem_tables), k_leaf_planes, k_examples --
at chosen states and edge geometries (tests/leaf_inputs_ref.py; test_leaf_inputs_cpu.py checks the inputs and references themselves).

One engine per geometry, one slot per state, sims = 2, RP_MOVE_EXTERNAL: rp_begin_episodes, rp_set_roots with the states, one
rp_search_step -- every state has a legal move, so every slot waits for the evaluator (n == games, asserted).

  a. planes     rp_leaf_planes row b == planes_from_state of state b bit for bit; rp_leaf_states returns what was set.
  b. integers   directed weight set, channels 0, 1, 2, 3, 5: rp_leaf_stem == float32(exact_stem) exactly; NCHW == channels-last,
                out_relu == relu(out); module set and back to the directed one: the same bits.
  c. reals      both weight sets, every element: |rp_leaf_stem - exact_stem| <= stem_tolerance, the header's "(N + 2) half units + half
                an ulp" plus the float64 reference's own rounding.  The bound is the documented one, not tuned to the figures below.
  d. rows       capacity_rows in {0, 1, n - 1, n, n + 5}, guarded buffers pre-filled with a sentinel, for rp_leaf_stem (both layouts,
                with and without out_relu) and rp_leaf_planes, LDS form (20x20/32) and L2 form (33x8/41); then slots that alternate between
                legal states and the terminal full board: identity rows (a non-waiting slot's row keeps the sentinel), compact rows.
  e. look-ahead 10x10/8 with games = 40 n_cu + 5 slots, every seventh terminal: the LDS form launches at most n_cu x STEM_WAVES workgroups
                of WAVES_PER_BLOCK waves, so while STEM_WAVES x WAVES_PER_BLOCK <= 12 (3 x 4 today) that is more than three strides of the
                persistent grid: every wave hands its look-ahead registers over at least three times, skips non-waiting slots and runs
                the tail where b + stride >= limit.  Every waiting row == the row of the same state in a 64-slot engine, bit for bit.
  f. replay     rp_expand_examples on a host-built packed set of the same states (counts up to 2^32 - 1, an example without counts, a
                repeated shuffled index list, index = NULL), and its guards: index -1, index E, sp_off + sp_n > S, sp_n < 0, action >= A.
                The packed arrays sit inside larger initialised allocations, so a guard that failed would show as a wrong row.

Paths taken, by the launcher's own formulas (leaf_inputs_ref.table_in_lds / corner_dims / small_items / persistent_trips): item table
in LDS for N <= 40 (seven geometries), in L2 for 33x8/41, 12x64/65, 63x64/64, 64x64/128; every geometry with N >= 4 has states with
at least four small unplaced items (corner phase taken) and states with fewer (not taken), 1x1/1 and 64x1/3 cannot take it; section e
gives every wave 4 leaves (3 or 4 in the last stride) on a 256-CU device.

Measured on an MI355X (256 CUs), section c, worst |error| / bound over all elements, directed set then module set, and the states
that take the corner phase:
    1x1/1      0.759  0.668   LDS  corner 8x2   0 of 16        33x8/41    0.284  0.274   L2   corner 8x8  10 of 16
    2x3/4      0.745  0.773   LDS  corner 8x2   3 of 16        64x1/3     0.804  0.841   LDS  corner 4x8   0 of 16
    6x5/5      0.770  0.789   LDS  corner 8x6   3 of 16        12x64/65   0.178  0.251   L2   corner 8x8  10 of 16
    20x20/32   0.334  0.368   LDS  corner 8x8   9 of 16        63x64/64   0.179  0.194   L2   corner 4x8  10 of 16
    32x9/40    0.277  0.319   LDS  corner 8x8  10 of 16        64x64/128  0.127  0.119   L2   corner 4x8  12 of 18
-- inside the bound everywhere; on the small geometries nearly all of it is the half ulp of the one conversion (a ratio near 1 is a
result rounded the other way, which the contract allows), on the large ones the quantisation term's worst case is far from reached.
The integer channels are exact at every geometry.  Every case runs in under a quarter of a second; section e took 0.18 s.

Found by this test: rp_create refused W = 1 ("internal: division magic") although the ABI allows 1 <= W: the self-check of the
multiply-shift division by W ran over 8192 values whatever the geometry, and for W = 1 the product leaves 32 bits from 4096 on.  The
check now covers what the kernels divide (actions below A, cell indices below H W rounded up to a wave); 1x1/1 pins it.
"""
import numpy as np
import pytest

import leaf_inputs_ref as ref

pytestmark = pytest.mark.gpu

G, TAIL = 2, 6  # guard rows before and after (capacity_rows goes up to n + 5: the rows behind must exist to be checked)
SENTINEL = 12345.0  # as test_gpu_stage_rows.py
SENTINEL_BITS = int(np.float32(SENTINEL).view(np.int32))
WORST = {}  # geometry -> {weight set: worst |error| / bound}


def _gid(g):
    return "%dx%d-%d" % tuple(g)


def _bits(t):
    import torch
    return t.view(torch.int32)


def _same_bits(a, b):
    import torch
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _holds_sentinel(t):
    return bool((_bits(t) == SENTINEL_BITS).all())


def _untouched(t):
    return not bool((_bits(t) == SENTINEL_BITS).any())


def _engine(W, H, N, rows, rem, wh):
    """An engine with one slot per state, rooted there.  A terminal root is accepted: its slot runs its two simulations without the
    evaluator and ends up RP_PHASE_MOVE_READY, never waiting."""
    import torch
    from resource_packing_self_play_amd import _lib
    n = len(rows)
    eng = _lib.Engine(W, H, N, n, 2, move_rule=_lib.MOVE_EXTERNAL, stream=torch.cuda.current_stream().cuda_stream)
    try:
        eng.begin_episodes(wh, np.full(n, W * H, np.int32))
        eng.set_roots(rows, rem)
    except Exception:
        eng.close()
        raise
    return eng


class _Weights:
    """a weight set on the device, alive until the tables are built"""

    def __init__(self, eng, name, N):
        import torch
        w, b = ref.WEIGHT_SETS[name](N)
        self.w, self.b = torch.from_numpy(w.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
        eng.stem_set_weights(self.w.data_ptr(), self.b.data_ptr())
        torch.cuda.synchronize()


def _guarded(rows, tail, nhwc=False):
    """A [G + rows + TAIL, ...] buffer of the sentinel (channels-last memory if nhwc) and its rows [G : G + rows]."""
    import torch
    buf = torch.full((G + rows + TAIL,) + tuple(tail), SENTINEL, device="cuda")
    if nhwc:
        buf = buf.contiguous(memory_format=torch.channels_last)
    return buf, buf[G:G + rows]


FORMS = [("stem", False, False), ("stem", False, True), ("stem", True, False), ("stem", True, True), ("planes", False, False)]


def _form_id(f):
    return f[0] + ("-nhwc" if f[1] else "") + ("-relu" if f[2] else "")


class _Runner:
    """rp_leaf_stem / rp_leaf_planes of one engine into guarded sentinel buffers"""

    def __init__(self, eng, rows):
        self.eng, self.rows = eng, rows
        self.Hp, self.Wp = (eng.H + 1) // 2, (eng.W + 1) // 2

    def run(self, form, capacity):
        """-> [(whole buffer, its rows [G : G + rows])] for out (and out_relu)"""
        import torch
        kind, nhwc, relu = form
        eng = self.eng
        if kind == "planes":
            outs = [_guarded(self.rows, (eng.N + 1, eng.H, eng.W))]
            eng.leaf_planes(outs[0][1].data_ptr(), capacity)
        else:
            outs = [_guarded(self.rows, (16, self.Hp, self.Wp), nhwc) for _ in range(2 if relu else 1)]
            eng.leaf_stem(outs[0][1].data_ptr(), capacity, outs[1][1].data_ptr() if relu else None, channels_last=nhwc)
        torch.cuda.synchronize()
        return outs


def _stem(eng, n, nhwc=False):
    """(out, out_relu) of rp_leaf_stem for n rows, both [n, 16, Hp, Wp]"""
    outs = _Runner(eng, n).run(("stem", nhwc, True), n)
    for buf, v in outs:
        assert _holds_sentinel(buf[:G]) and _holds_sentinel(buf[G + n:]) and _untouched(v)
    return outs[0][1], outs[1][1]


# ---- one engine per geometry: sections a, b, c, f ------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=ref.GEOMETRIES, ids=_gid)
def geo(request):
    W, H, N = request.param
    st = ref.states(W, H, N)
    eng = _engine(W, H, N, st.rows, st.rem, st.wh)
    n = eng.search_step()
    small = [ref.small_items(st.rem[k], st.wh[k], W) for k in range(len(st))]
    print("\n%s: item table in %s, corner %dx%d taken by %d of %d states, %d pass(es) per leaf" % (
        _gid(request.param), "LDS" if ref.table_in_lds(N) else "L2", *ref.corner_dims(W), sum(s >= ref.CORNER_MIN_ITEMS for s in small), len(st),
        ref.stem_passes(W, H)))
    yield dict(geometry=request.param, st=st, eng=eng, n=n)
    eng.close()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nsection c, worst |error| / bound (directed, module):")
        for g in ref.GEOMETRIES:
            if g in WORST:
                print("    %-12s %.3f  %.3f" % (_gid(g), WORST[g].get("directed", float("nan")), WORST[g].get("module", float("nan"))))


def test_planes_and_states_of_every_slot(geo):
    import torch
    st, eng, n = geo["st"], geo["eng"], geo["n"]
    assert n == len(st), "a state was skipped"
    rows, rem, slots = eng.leaf_states(n)
    assert np.array_equal(slots, np.arange(n)) and np.array_equal(rows, st.rows) and np.array_equal(rem, st.rem)
    (buf, planes), = _Runner(eng, n).run(("planes", False, False), n)
    assert _holds_sentinel(buf[:G]) and _holds_sentinel(buf[G + n:])
    want = torch.from_numpy(st.planes()).cuda()
    assert _same_bits(planes, want)


def test_stem_integer_channels_are_exact(geo):
    import torch
    st, eng, n = geo["st"], geo["eng"], geo["n"]
    W, H, N = geo["geometry"]
    assert n == len(st), "a state was skipped"
    _Weights(eng, "directed", N)
    out, out_relu = _stem(eng, n)
    ch = list(ref.INTEGER_CHANNELS)
    want = ref.exact_stem_of(geo["geometry"], "directed")[:, ch].astype(np.float32)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.array_equal(got[:, ch], want), "channels %s differ" % sorted({ch[c] for c in np.nonzero(got[:, ch] != want)[1]})
    cl, cl_relu = _stem(eng, n, nhwc=True)
    assert cl.is_contiguous(memory_format=torch.channels_last) and _same_bits(cl, out) and _same_bits(cl_relu, out_relu)
    assert _same_bits(out_relu, torch.relu(out))
    _Weights(eng, "module", N)
    other, _ = _stem(eng, n)
    assert not _same_bits(other, out)
    _Weights(eng, "directed", N)
    again, again_relu = _stem(eng, n)
    assert _same_bits(again, out) and _same_bits(again_relu, out_relu)


@pytest.mark.parametrize("weights", ["directed", "module"])
def test_stem_within_the_documented_bound(geo, weights):
    st, eng, n = geo["st"], geo["eng"], geo["n"]
    W, H, N = geo["geometry"]
    assert n == len(st), "a state was skipped"
    _Weights(eng, weights, N)
    out, _ = _stem(eng, n)
    g = out.cpu().numpy().astype(np.float64)
    y = ref.exact_stem_of(geo["geometry"], weights)
    B, q = ref.stem_bound_of(N, weights)
    tol = ref.stem_tolerance(B, q, N, y, g)
    err = np.abs(g - y)
    ratio = err / tol
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print("%s %s: worst |error| / bound %.3f (|error| %.3e, bound %.3e, state %d channel %d pixel (%d, %d)); per channel %s" % (
        _gid(geo["geometry"]), weights, ratio[at], err[at], tol[at], *at, " ".join("%.2f" % v for v in ratio.max(axis=(0, 2, 3)))))
    WORST.setdefault(geo["geometry"], {})[weights] = float(ratio[at])
    assert (err <= tol).all()


# ---- f. replay expansion ---------------------------------------------------------------------------------------------------------
E_PAD, S_PAD = 2, 96  # initialised slack, in examples and in pool entries, on both sides of every packed array


class _Packed:
    """A packed set inside larger initialised allocations: the slack examples are copies of real ones that point at real pool entries,
    the slack pool entries are valid pairs -- whatever a failed guard read there would expand to a non-zero row."""

    def __init__(self, d, A):
        import torch
        E, S = len(d["sp_n"]), len(d["sp_act"])
        rng = np.random.default_rng(E + S)

        def ex(a):  # slack examples: real ones, rolled
            return np.concatenate([np.roll(a, 1, axis=0)[:E_PAD], a, np.roll(a, -1, axis=0)[-E_PAD:]])
        off = ex(d["sp_off"])
        nn = ex(d["sp_n"])
        nn[:E_PAD] = np.maximum(nn[:E_PAD], 1); nn[-E_PAD:] = np.maximum(nn[-E_PAD:], 1)
        self.host = dict(key=ex(d["key"]), wh=ex(d["wh"]), value=np.concatenate([[1] * E_PAD, d["value"], [-1] * E_PAD]).astype(np.int32),
                         sp_off=off.astype(np.int64), sp_n=nn.astype(np.int32),
                         sp_act=np.concatenate([rng.integers(0, A, S_PAD), d["sp_act"], rng.integers(0, A, S_PAD)]).astype(np.uint16),
                         sp_cnt=np.concatenate([rng.integers(1, 99, S_PAD), d["sp_cnt"], rng.integers(1, 99, S_PAD)]).astype(np.uint32))
        view = dict(sp_act=np.int16, sp_cnt=np.int32, key=np.int32)
        self.dev = {k: torch.from_numpy(v.view(view[k]) if k in view else v).cuda() for k, v in self.host.items()}
        self.E, self.S = E, S

    def args(self):
        """the tensors rp_expand_examples gets: the middle of every allocation"""
        t, E, S = self.dev, self.E, self.S
        ex = lambda k: t[k][E_PAD:E_PAD + E]
        return [ex("key"), ex("wh"), ex("value"), ex("sp_off"), ex("sp_n"), t["sp_act"][S_PAD:S_PAD + S], t["sp_cnt"][S_PAD:S_PAD + S]]


def _expand(eng, packed, index):
    """-> planes, pi, value (numpy) of rp_expand_examples for the index list (None: every example in order); no check yet"""
    import torch
    n = packed.E if index is None else len(index)
    nan = float("nan")
    planes = torch.full((n, eng.N + 1, eng.H, eng.W), nan, device="cuda")
    pi = torch.full((n, eng.A), nan, device="cuda")
    value = torch.full((n,), nan, device="cuda")
    idx = None if index is None else torch.from_numpy(np.asarray(index, np.int64)).cuda()
    torch.cuda.synchronize()
    eng.expand_examples(idx, *packed.args(), planes, pi, value)
    return planes, pi, value


def _rows_equal(got, want_planes, want_pi, want_value, rows=None):
    planes, pi, value = (t.cpu().numpy() for t in got)
    rows = range(len(value)) if rows is None else rows
    for k in rows:
        assert np.array_equal(planes[k].view(np.int32), want_planes[k].view(np.int32)), "planes of row %d" % k
        assert np.array_equal(pi[k].view(np.int32), want_pi[k].view(np.int32)), "pi of row %d" % k
        assert value[k] == want_value[k], "value of row %d" % k


def test_replay_expansion_and_its_guards(geo):
    from resource_packing_self_play_amd import _lib
    st, eng = geo["st"], geo["eng"]
    W, H, N = geo["geometry"]
    A, E = W * N, len(st)
    d = ref.packed_set(W, H, N)
    S = len(d["sp_act"])
    assert d["key"].shape == (E, eng.KW) and int(d["sp_cnt"].max()) == 2 ** 32 - 1 and d["sp_n"][1] == 0 and int(d["sp_n"].sum()) == S
    all_planes = st.planes()
    all_pi = np.stack([ref.expected_pi(d, A, e) for e in range(E)])
    all_value = d["value"].astype(np.float32)
    assert not all_pi[1].any() and abs(float(all_pi[0].sum()) - 1) < 1e-5
    packed = _Packed(d, A)
    rng = np.random.default_rng(E + A)
    index = rng.permutation(np.concatenate([np.arange(E), rng.integers(0, E, 5)]))  # every example, five of them twice, shuffled
    for idx in (None, index):
        got = _expand(eng, packed, idx)
        eng.check()  # rp_check == 0
        sel = np.arange(E) if idx is None else idx
        _rows_equal(got, all_planes[sel], all_pi[sel], all_value[sel])

    def guard_case(packed, idx, bad_row, want_bad_pi=None):
        """row bad_row is zero (or has want_bad_pi), the others are right, rp_check reports RP_ERR_ARG once"""
        got = _expand(eng, packed, idx)
        with pytest.raises(_lib.EngineError) as err:
            eng.check()
        assert err.value.code == _lib.ERR_ARG
        eng.check()  # reported once
        sel = np.where((idx >= 0) & (idx < E), idx, 0)
        want = [all_planes[sel], all_pi[sel], all_value[sel]]
        if want_bad_pi is None:
            want = [w.copy() for w in want]
            for w in want:
                w[bad_row] = 0
        else:
            want[1] = want[1].copy()
            want[1][bad_row] = want_bad_pi
        _rows_equal(got, *want)

    for bad in (-1, E):  # an index outside the set
        idx = index.copy()
        idx[3] = bad
        guard_case(packed, idx, 3)
    victim = 0  # an example with counts
    assert d["sp_n"][victim] > 0
    for field, value in (("sp_off", S - int(d["sp_n"][victim]) + 1), ("sp_n", S - int(d["sp_off"][victim]) + 1), ("sp_n", -1)):
        bad = {k: v.copy() for k, v in d.items()}
        bad[field][victim] = value  # sp_off + sp_n == S + 1, twice; a negative sp_n
        idx = index.copy()
        guard_case(_Packed(bad, A), idx, np.nonzero(index == victim)[0])
    bad = {k: v.copy() for k, v in d.items()}
    at = int(d["sp_off"][victim]) + int(d["sp_n"][victim]) - 1  # the example's last pair names action A
    lost = int(bad["sp_act"][at])
    bad["sp_act"][at] = A
    want = all_pi[victim].copy()
    want[lost] = 0  # only that entry is missing: the others still divide by the sum of all counts
    guard_case(_Packed(bad, A), index.copy(), np.nonzero(index == victim)[0], want_bad_pi=want)


# ---- d. row contract ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", [(20, 20, 32), (33, 8, 41)], ids=_gid)
def test_row_contract(geometry):
    import torch
    from resource_packing_self_play_amd import _lib
    W, H, N = geometry
    st = ref.states(W, H, N)
    n = len(st)
    assert ref.table_in_lds(N) == (geometry == (20, 20, 32))
    eng = _engine(W, H, N, st.rows, st.rem, st.wh)
    full = {}
    try:
        assert eng.search_step() == n
        _Weights(eng, "module", N)
        run = _Runner(eng, n)
        for form in FORMS:
            outs = run.run(form, n)
            for buf, v in outs:
                assert _holds_sentinel(buf[:G]) and _holds_sentinel(buf[G + n:]), "%s: a guard row was written" % _form_id(form)
                assert _untouched(v), "%s: a row was not written" % _form_id(form)
            full[form] = [v.clone(memory_format=torch.preserve_format) for _, v in outs]
            for cap in (0, 1, n - 1, n, n + 5):
                m = min(cap, n)
                for (buf, v), want in zip(run.run(form, cap), full[form]):
                    assert _same_bits(v[:m], want[:m]), "%s capacity %d: a row below the capacity differs from the full run" % (_form_id(form), cap)
                    assert _holds_sentinel(buf[:G]) and _holds_sentinel(buf[G + m:]), "%s capacity %d: a row from the capacity on was written" % (_form_id(form), cap)
    finally:
        eng.close()
    # the full run is what sections a to c hold to the references
    assert _same_bits(full[FORMS[4]][0], torch.from_numpy(st.planes()).cuda())
    y = ref.exact_stem_of(geometry, "module")
    g = full[FORMS[0]][0].cpu().numpy().astype(np.float64)
    assert (np.abs(g - y) <= ref.stem_tolerance(*ref.stem_bound_of(N, "module"), N, y, g)).all()
    for form in FORMS[1:4]:
        assert _same_bits(full[form][0], full[FORMS[0]][0])
    for form in (FORMS[1], FORMS[3]):
        assert _same_bits(full[form][1], torch.relu(full[FORMS[0]][0]))

    # slots that alternate between a legal state and the terminal full board: the waiting slots are not a prefix
    rows2 = st.rows.copy()
    rows2[1::2] = ref.terminal_rows(W, H)
    wait = np.arange(0, n, 2)
    eng = _engine(W, H, N, rows2, st.rem, st.wh)
    try:
        eng.search_step(sync=False)  # identity rows: row b belongs to slot b
        eng.check()
        phase = eng.status()[0]
        assert (phase[wait] == _lib.PHASE_WAIT_EVAL).all() and (phase[1::2] != _lib.PHASE_WAIT_EVAL).all()
        _Weights(eng, "module", N)
        run = _Runner(eng, n)
        for form in FORMS:
            for (buf, v), want in zip(run.run(form, n), full[form]):
                assert _same_bits(v[0::2], want[0::2]), "%s: a waiting slot's row differs from the same state's row in the full run" % _form_id(form)
                assert _holds_sentinel(v[1::2]) and _holds_sentinel(buf[:G]) and _holds_sentinel(buf[G + n:]), "%s: a non-waiting slot's row was written" % _form_id(form)
        eng.set_compact_rows(True)
        eng.search_step(sync=False)  # lists the waiting slots on the device: row b belongs to the b-th of them
        cnt = len(wait)
        for form in FORMS:
            for cap in (n, cnt, 3):
                m = min(cap, cnt)
                for (buf, v), want in zip(run.run(form, cap), full[form]):
                    assert _same_bits(v[:m], want[0::2][:m]), "%s compact, capacity %d: row b is not the b-th waiting slot's" % (_form_id(form), cap)
                    assert _holds_sentinel(buf[:G]) and _holds_sentinel(buf[G + m:]), "%s compact, capacity %d: a row from the count on was written" % (_form_id(form), cap)
    finally:
        eng.close()


# ---- e. look-ahead pipeline of the persistent waves ------------------------------------------------------------------------------
def test_lookahead_pipeline_over_more_than_three_strides():
    import torch
    from resource_packing_self_play_amd import _lib
    W, H, N = ref.PIPELINE_GEOMETRY
    assert ref.table_in_lds(N)
    n_cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    games = 40 * n_cu + 5
    trips = ref.persistent_trips(games, n_cu)
    print("\n%d CUs, %d slots: up to %d leaves per wave" % (n_cu, games, trips))
    assert trips >= 4
    st = ref.states(W, H, N, ref.PIPELINE_STATES)
    assert len({(st.rows[k].tobytes(), st.rem[k].tobytes(), st.wh[k].tobytes()) for k in range(len(st))}) == ref.PIPELINE_STATES
    eng = _engine(W, H, N, st.rows, st.rem, st.wh)
    try:
        assert eng.search_step() == len(st)
        _Weights(eng, "module", N)
        want = {False: [t.clone(memory_format=torch.preserve_format) for t in _stem(eng, len(st), nhwc=False)],
                True: [t.clone(memory_format=torch.preserve_format) for t in _stem(eng, len(st), nhwc=True)]}
    finally:
        eng.close()
    order, terminal = ref.pipeline_slots(games)
    rows = st.rows[order].copy()
    rows[terminal] = ref.terminal_rows(W, H)
    wait = np.nonzero(~terminal)[0]
    eng = _engine(W, H, N, rows, st.rem[order], st.wh[order])
    try:
        eng.search_step(sync=False)  # identity rows
        eng.check()
        phase = eng.status()[0]
        assert (phase[wait] == _lib.PHASE_WAIT_EVAL).all() and (phase[terminal] != _lib.PHASE_WAIT_EVAL).all()
        _Weights(eng, "module", N)
        run = _Runner(eng, games)
        dev = lambda a: torch.from_numpy(np.asarray(a)).cuda()
        src, wait_d, term_d = dev(order[wait]), dev(wait), dev(np.nonzero(terminal)[0])
        for nhwc in (False, True):
            form = ("stem", nhwc, True)
            for cap in (games, games - 3):  # identity rows
                m = int((wait < cap).sum())
                for (buf, v), ref_rows in zip(run.run(form, cap), want[nhwc]):
                    assert _same_bits(v[wait_d[:m]], ref_rows[src[:m]]), "identity rows, capacity %d: a waiting row differs from its state's row in the 64-slot engine" % cap
                    assert _holds_sentinel(v[term_d]) and _holds_sentinel(v[wait_d[m:]]) and _holds_sentinel(buf[:G]) and _holds_sentinel(buf[G + cap:])
        eng.set_compact_rows(True)
        eng.search_step(sync=False)
        cnt = len(wait)
        for nhwc in (False, True):
            form = ("stem", nhwc, True)
            for cap in (games, games - 3, cnt - 3):
                m = min(cap, cnt)
                for (buf, v), ref_rows in zip(run.run(form, cap), want[nhwc]):
                    assert _same_bits(v[:m], ref_rows[src[:m]]), "compact rows, capacity %d: row b is not the b-th waiting slot's" % cap
                    assert _holds_sentinel(buf[:G]) and _holds_sentinel(buf[G + m:])
    finally:
        eng.close()
