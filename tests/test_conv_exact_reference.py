"""Host checks of the exact-arithmetic convolution tests (tests/test_gpu_conv_exact.py): for every row of every case table,
the conditions that make a zero-tolerance comparison legitimate, and a self-test that the data can see the bugs the
tolerance tests cannot.

Per expectation: sum|terms| / unit < 2^24 on every element and the fp64 reference is an fp32 number (to_store asserts
both); for bf16-stored outputs at most 1 % of the elements are changed by the one bf16 rounding, so that a rounding cannot
hide a +-1 error on more than a sliver of the output; every ReLU / LeakyReLU mask holds 25 - 75 % of each sign; the hi + lo
operands have non-zero lo parts and their three-term reference differs from the hi-only product."""
import collections

import pytest
import torch

import conv_exact_util as U

BF16_ALTERED_CAP = 0.01


def test_value_sets_hold_no_zero_and_hilo_splits_without_rounding():
    for vals in (U.PM1, U.BIAS_VALS, U.SCALE_VALS):
        assert 0 not in vals
    v = U.hilo((4, 5, 6), 3)
    hi, lo = U.split(v)
    assert set(hi.unique().tolist()) == {-1.0, 1.0}
    assert set(lo.unique().tolist()) == {-U.LO_UNIT, U.LO_UNIT}
    assert torch.equal(U.ints((3, 4), 7), U.ints((3, 4), 7)) and not torch.equal(U.ints((30, 40), 7), U.ints((30, 40), 8))


def test_every_case_table_meets_the_exactness_conditions():
    worst = collections.defaultdict(lambda: [0.0, 0.0, 0])      # table -> [max sum|terms| / unit, max bf16-altered share, n]
    for table, row, e in U.all_expectations():
        for key, (val, mag, unit, kind) in e.wants.items():
            stored = e.stored(key)                               # asserts the 2^24 bound and fp32 representability
            w = worst[table]
            w[0] = max(w[0], float(mag.max()) / unit)
            w[2] += 1
            if kind == "bf16":
                w[1] = max(w[1], stored[1])
                assert stored[1] <= BF16_ALTERED_CAP, f"{table} {row} {key}: bf16 rounding alters {stored[1]:.2%} of the elements"
            elif kind == "split":
                hi, lo = stored                                  # the same cap for the two roundings of a split store
                share = (hi.double() + lo.double() != val).double().mean().item()
                w[1] = max(w[1], share)
                assert share <= BF16_ALTERED_CAP, f"{table} {row} {key}: the split store alters {share:.2%} of the elements"
        for name, t in e.masks.items():
            s = U.sign_share(t)
            assert 0.25 <= s <= 0.75, f"{table} {row}: mask '{name}' is {s:.1%} positive"
    for table, (m, share, n) in sorted(worst.items()):
        print(f"{table}: {n} comparisons, max sum|terms| / unit = {m:.0f} (2^24 = {2 ** 24}), bf16-altered share <= {share:.3%}")
    assert set(worst) == {"halo", "generic", "descriptor", "1x1", "nhwc_s1", "nhwc_s2", "ops", "wgrad3", "wgrad1", "im2col",
                          "linear", "stem"}


@pytest.mark.parametrize("op", ["fwd", "dgrad", "wgrad"])
def test_hilo_operands_make_the_lo_planes_count(op):
    a, b = U.hilo((2, 24, 9, 11), 11), U.hilo((24, 40, 3, 3), 12)
    x = U.hilo((2, 40, 9, 11), 13)
    fn, p, q = {"fwd": (lambda u, v: U.conv(u, v, 1, 1), x, b),
                "dgrad": (lambda u, v: U.conv_in(u, v, (9, 11), 1, 1), a, b),
                "wgrad": (lambda u, v: U.conv_w(u, v, 3, 1, 1), a, x)}[op]
    (ph, pl), (qh, ql) = U.split(p), U.split(q)
    assert pl.abs().min() > 0 and ql.abs().min() > 0
    three = U.three_term(fn, p, q)
    assert not torch.equal(three, fn(ph, qh)), "the lo planes do not reach the reference"
    full = fn(p, q)
    assert torch.equal(three + fn(pl, ql), full), "three-term sum + lo * lo must be the full product"
    assert not torch.equal(three, full), "the reference must NOT hold the lo * lo term"
    # dropping either cross term is visible on every element pattern the kernel could drop it for
    assert not torch.equal(three, fn(ph, qh) + fn(pl, qh)) and not torch.equal(three, fn(ph, qh) + fn(ph, ql))


def test_the_data_sees_a_dropped_product_a_shifted_column_and_a_dropped_lo_term():
    B, Cin, H, W, Cout = 1, 72, 17, 65, 184
    x, w = U.ints((B, Cin, H, W), 21), U.ints((Cout, Cin, 3, 3), 22)
    ref = U.conv(x, w, 1, 1)
    # one (channel, tap) product dropped: the last channel of the ragged third chunk, for one output channel
    w1 = w.clone()
    w1[5, Cin - 1, 2, 0] = 0
    d = U.conv(x, w1, 1, 1) != ref
    assert d.any() and not d[:, :5].any() and not d[:, 6:].any()
    assert d[:, 5, :-1, 1:].all(), "every element that tap reaches in that output channel changes by +-1"
    # one patch column read one pixel off at the 32-pixel tile seam: column 32 of the input replaced by column 31
    x1 = x.clone()
    x1[..., 32] = x[..., 31]
    d = U.conv(x1, w, 1, 1) != ref
    assert d.any() and not d[..., :31].any() and not d[..., 34:].any()
    # one tap skipped for one output parity class of a strided data gradient
    dy, w4 = U.ints((1, 8, 6, 5), 23), U.ints((8, 5, 4, 4), 24)
    dref = U.conv_in(dy, w4, (13, 11), 2, 1)
    w5 = w4.clone()
    w5[:, :, 3, 1] = 0                                   # tap (3, 1) reaches input rows of parity 0, columns of parity 0
    d = U.conv_in(dy, w5, (13, 11), 2, 1) != dref
    assert d.any() and not d[..., 1::2, :].any() and not d[..., :, 1::2].any()
    # one lo * hi product dropped for one fragment (16 channels of one chunk)
    xs, ws = U.hilo((1, 40, 9, 33), 25), U.hilo((24, 40, 3, 3), 26)
    three = U.three_term(lambda u, v: U.conv(u, v, 1, 1), xs, ws)
    xh, xl = U.split(xs)
    wh, wl = U.split(ws)
    xl[:, 16:32] = 0
    dropped = U.conv(xh, wh, 1, 1) + U.conv(xl, wh, 1, 1) + U.conv(xh, wl, 1, 1)
    assert (dropped != three).double().mean() > 0.5


def test_to_store_rejects_data_that_is_not_exact():
    big = torch.full((2, 2), 2.0 ** 24)
    with pytest.raises(AssertionError):
        U.to_store(big.double(), "f32", big.double())
    with pytest.raises(AssertionError):
        U.to_store(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64), "f32", torch.tensor([2.0]))
    b, share = U.to_store(torch.tensor([257.0, 256.0], dtype=torch.float64), "bf16", torch.tensor([300.0]))
    assert b.float().tolist() == [256.0, 256.0] and share == 0.5
    hi, lo = U.to_store(torch.tensor([256.5 + 2.0 ** -10], dtype=torch.float64), "split", torch.tensor([300.0]), U.LO_UNIT)
    assert hi.item() == 256.0 and lo.item() == 0.5          # the 2^-10 does not fit 16 mantissa bits: the split drops it
