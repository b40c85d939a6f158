"""Probe policies: ONNX graphs whose exact answer is known without the oracle.

Two kinds, both written with the repository's own onnx_writer and handed to Engine as
bytes (plain numpy here; `oracle` is not imported, so the oracle gets a pin that does
not come from itself, tests/test_cpu_probe.py):

* Integer probes (`int_policy`): small integer weights, biases and observations.
  While `abs_sum_bound` < 2^24 every partial sum of every layer is an integer (or a
  dyadic fraction, see `frac_bits`) that float32 holds exactly, in any summation order:
  a kernel's answer must be `np.array_equal` to `int_ref`. There is no tolerance, so a
  form that drops one term, reads a stale row or leaves a row unswept fails, which a
  normwise 1e-5 against random float weights may not see.
* Activation probes (`act_policy`): identity layers around one activation, so output j
  of a row is act(x[j]) (composed d times when d hidden layers carry it); every other
  product is 0 * finite = 0. The reference (`act_ref`) is the ONNX formula in float64
  per element.

Out of scope, because the observation cannot be injected exactly through them: the dense
chain behind a GRU / LSTM cell, the controller-tick forms (an assembled observation) and
LayerNormalization epilogues (a normalisation). Multi-GPU and timing are not probed.
(The recurrent cell's own chunk walk is pinned against the fp64 oracle at every observation
width and instantiation by tests/test_gpu_rnn_widths.py.)

Points of the activation probes: +-0, then +- each of POINTS, the Clip bounds with their
float32 neighbours, and HardSigmoid's two corners. Subnormal inputs and |x| >= 2^126 are
left out: what the MFMA and v_rcp_f32 do with subnormal values (flush or keep) is a
property of the hardware, not of this code, 1 + |x| of Softsign must stay below the
reciprocal's flush range, and no policy pre-activation gets there.
"""
import numpy as np

from go2_onnx_controller_amd import onnx_writer as ow

# ---------------------------------------------------------------------------------------
# integer probes

SMALL_SCHEDULE = [8, 1, 5, 7, 4, 8]     # batch <= 8 forms: stale rows of a larger request are met
BATCH_SCHEDULE = [33, 1, 16, 17, 15]    # batched forms: 3 tiles with a ragged one, one row, a full tile

INT_ACTS = {"Relu": {}, "LeakyRelu": {"alpha": 0.5}, "Elu": {"alpha": 1.0}, "Clip": (0.0, float(2 ** 20))}


def _hidden_weights(N, K, l, signed):
    """[N, K] int64: row n has nnz = max(3, ceil(K / N)) (at most K) non-zero weights of
    magnitude 1-2 in the columns (nnz * n + j + 5 * l) mod K, j < nnz: consecutive blocks that
    walk over every input column (nnz * N >= K), shifted per layer. Signed probes: the
    first weight of a row is positive, the others alternate with (n, j, l)."""
    nnz = min(K, max(3, -(-K // N)))
    W = np.zeros((N, K), np.int64)
    n = np.arange(N)
    for j in range(nnz):
        col = (nnz * n + j + 5 * l) % K
        mag = 1 + (n + j + l) % 2
        sgn = np.where((j > 0) & ((n // 2 + j + l) % 2 == 1), -1, 1) if signed else 1
        W[n, col] = mag * sgn
    return W


def _head_weights(N, K, signed):
    """[N, K] int64, dense in {-1, 0, 1} (signed) or {0, 1}; every column has a non-zero."""
    n, k = np.arange(N)[:, None], np.arange(K)[None, :]
    h = (n * 31 + k * 17 + (n * k) % 13)
    W = (h % 3 - 1) if signed else (h % 2)
    W = W.astype(np.int64)
    dead = np.flatnonzero((W != 0).sum(0) == 0)
    W[dead % N, dead] = 1
    return W


def int_inputs(layers, schedule, seed=0):
    """One float32 observation array per request of `schedule`: the integers of the probe's
    range ([-3, 3] signed, [0, 3] non-negative) in front of its front-end, if it has one."""
    r = np.random.default_rng(7000 + seed + 13 * layers["dims"][0] + len(layers["dims"]))
    K, signed, front = layers["dims"][0], layers["signed"], layers["front"]
    out = []
    for B in schedule:
        if front is None:
            x = r.integers(-3 if signed else 0, 4, (B, K))
        else:   # (obs - sub) * 0.5 is a half-integer in [-3, 3] / [0, 3]
            x = r.integers(-6 if signed else 0, 7, (B, K)) + front[0]
        out.append(x.astype(np.float32))
    return out


def int_policy(dims, act, signed, front=False, tail=False):
    """(onnx bytes, layers) of the integer probe dims[0] -> ... -> dims[-1] with activation
    `act` (a key of INT_ACTS) after every hidden layer. signed=False: weights, biases and
    observations are non-negative, so every pre-activation is >= 0, where Elu (alpha 1) is
    the identity and Elu(0) = 0 exactly. front: a per-column Sub of integers and a Mul by
    0.5 in front of layer 0; tail: a Clip on the head's output that binds on some outputs of
    the probe's schedules (its bounds: the quartiles of the un-clipped reference answer),
    then a Mul by 0.25. `layers` is what int_ref / abs_sum_bound take."""
    dims = list(dims)
    assert act in INT_ACTS and (signed or act in ("Elu", "Clip")) and (act != "Elu" or not signed)
    nl = len(dims) - 1
    dense = []
    for l, (K, N) in enumerate(zip(dims[:-1], dims[1:])):
        n = np.arange(N)
        if l == nl - 1:
            W, b = _head_weights(N, K, signed), (n % 5 - 2 if signed else n % 3).astype(np.int64)
        else:  # hidden biases 1..3: no unit is identically zero
            W, b = _hidden_weights(N, K, l, signed), (1 + (n + l) % 3).astype(np.int64)
        dense.append({"W": W, "b": b, "act": None if l == nl - 1 else act})
    layers = {"dims": dims, "signed": signed, "act": act, "dense": dense, "front": None, "tail": None}
    if front:
        layers["front"] = ((np.arange(dims[0]) % 7 - 3).astype(np.int64), 0.5)
    if tail:
        xs = np.concatenate(int_inputs(layers, SMALL_SCHEDULE + BATCH_SCHEDULE))
        y = np.asarray(int_ref(layers, xs), np.float64)
        lo, hi = np.floor(np.percentile(y, 25)), np.ceil(np.percentile(y, 75))
        layers["tail"] = (float(lo), float(max(hi, lo + 1)), 0.25)

    nodes, inits, cur = [], [], "obs"
    if front:
        inits += [("pre_sub", layers["front"][0].astype(np.float32)), ("pre_mul", np.array(0.5, np.float32))]
        nodes += [ow.node("Sub", ["obs", "pre_sub"], ["x_c"]), ow.node("Mul", ["x_c", "pre_mul"], ["x_n"])]
        cur = "x_n"
    for l, d in enumerate(dense):
        inits += [(f"W{l}", d["W"].astype(np.float32)), (f"b{l}", d["b"].astype(np.float32))]
        nodes.append(ow.node("Gemm", [cur, f"W{l}", f"b{l}"], [f"g{l}"], "", [ow.attr_int("transB", 1)]))
        cur = f"g{l}"
        if d["act"] == "Clip":
            inits += [(f"lo{l}", np.array(INT_ACTS["Clip"][0], np.float32)),
                      (f"hi{l}", np.array(INT_ACTS["Clip"][1], np.float32))]
            nodes.append(ow.node("Clip", [cur, f"lo{l}", f"hi{l}"], [f"a{l}"]))
            cur = f"a{l}"
        elif d["act"]:
            nodes.append(ow.node(d["act"], [cur], [f"a{l}"], "",
                                 [ow.attr_float(k, v) for k, v in INT_ACTS[d["act"]].items()]))
            cur = f"a{l}"
    if tail:
        lo, hi, k = layers["tail"]
        inits += [("t_lo", np.array(lo, np.float32)), ("t_hi", np.array(hi, np.float32)), ("t_k", np.array(k, np.float32))]
        nodes += [ow.node("Clip", [cur, "t_lo", "t_hi"], ["t_c"]), ow.node("Mul", ["t_c", "t_k"], ["t_s"])]
        cur = "t_s"
    nodes.append(ow.node("Identity", [cur], ["act"]))
    return ow.model(nodes, inits, [("obs", ["N", dims[0]])], [("act", ["N", dims[-1]])]), layers


def _int_forward(layers, x, zero=None):
    """Per-layer values of the probe on observations x: [(pre-activation, activation)].
    int64 where every value is an integer, float64 (exact: dyadic fractions far inside 53
    bits) with a front-end, a tail or LeakyRelu. zero = (l, j): unit j of layer l's output
    (l = -1: observation column j, after the front-end) is replaced by 0."""
    frac = layers["front"] is not None or layers["act"] == "LeakyRelu"
    dt = np.float64 if frac else np.int64
    x = np.asarray(x)
    assert np.array_equal(x, np.round(x))
    h = x.astype(np.int64)
    if layers["front"] is not None:
        h = (h - layers["front"][0]).astype(np.float64) * layers["front"][1]
    h = h.astype(dt)
    if zero is not None and zero[0] == -1:
        h = h.copy()
        h[:, zero[1]] = 0
    out = []
    for l, d in enumerate(layers["dense"]):
        z = h @ d["W"].T.astype(dt) + d["b"].astype(dt)
        if d["act"] is None:
            a = z
        elif d["act"] == "Relu":
            a = np.maximum(z, 0)
        elif d["act"] == "LeakyRelu":
            a = np.where(z >= 0, z, 0.5 * z)
        elif d["act"] == "Elu":
            assert (z >= 0).all(), "a non-negative probe with a negative pre-activation"
            a = z
        else:
            a = np.clip(z, int(INT_ACTS["Clip"][0]), int(INT_ACTS["Clip"][1]))
        if zero is not None and zero[0] == l:
            a = a.copy()
            a[:, zero[1]] = 0
        out.append((z, a))
        h = a
    return out


def int_ref(layers, x, zero=None):
    """The probe's exact answer on x [B, in]: int64, or float64 on values exact there."""
    y = _int_forward(layers, x, zero)[-1][1]
    if layers["tail"] is not None:
        lo, hi, k = layers["tail"]
        y = np.clip(y.astype(np.float64), lo, hi) * k
    return y


def _act64(name, z):
    if name is None:
        return z
    if name == "Relu":
        return np.maximum(z, 0)
    if name == "LeakyRelu":
        return np.where(z >= 0, z, 0.5 * z)
    if name == "Elu":
        return z
    return np.clip(z, *INT_ACTS["Clip"])


def unobserved(layers, xs, chunk=128):
    """The (layer, unit) pairs (layer -1: observation columns) whose zeroing changes no output
    of any row of xs: [] is what the tests require of every probe and schedule. A
    non-negative probe without a tail is monotone (weights >= 0, the activation the identity
    on its range), so a unit is observed iff it is positive in some row and the next layer
    has a positive weight on it, which is checked structurally; every other probe is
    measured by zeroing each unit in turn (float64, exact on these values)."""
    vals = _int_forward(layers, xs)
    dense = layers["dense"]
    h0 = np.asarray(xs, np.float64)
    if layers["front"] is not None:
        h0 = (h0 - layers["front"][0]) * layers["front"][1]
    acts = [h0] + [np.asarray(a, np.float64) for _, a in vals]
    missing = []
    if not layers["signed"] and layers["act"] == "Elu" and layers["tail"] is None:
        for l in range(len(dense)):
            live = (acts[l] > 0).any(0) & ((dense[l]["W"] > 0).any(0))
            missing += [(l - 1, int(j)) for j in np.flatnonzero(~live)]
        return missing
    base = np.asarray(int_ref(layers, xs), np.float64)
    for l in range(len(dense)):           # zero a unit of acts[l] (the input of layer l)
        n = acts[l].shape[1]
        for u0 in range(0, n, chunk):
            u = np.arange(u0, min(n, u0 + chunk))
            h = np.repeat(acts[l][None], len(u), 0)       # [units, rows, width]
            h[np.arange(len(u)), :, u] = 0
            for m in range(l, len(dense)):
                h = _act64(dense[m]["act"], h @ dense[m]["W"].T.astype(np.float64) + dense[m]["b"])
            if layers["tail"] is not None:
                h = np.clip(h, layers["tail"][0], layers["tail"][1]) * layers["tail"][2]
            same = (h == base[None]).all((1, 2))
            missing += [(l - 1, int(j)) for j in u[same]]
    return missing


def frac_bits(layers):
    """Fractional bits a value inside the probe can carry: 1 after the front-end's Mul by
    0.5, 1 more per LeakyRelu(0.5) layer (the tail's Mul by 0.25 is one exact scaling of
    the answer and adds none to a sum)."""
    n = 1 if layers["front"] is not None else 0
    return n + (len(layers["dense"]) - 1 if layers["act"] == "LeakyRelu" else 0)


def abs_sum_bound(layers, x):
    """The largest sum |w| |h| + |b| over all layers, output units and rows of x, in units of
    the probe's smallest fractional bit (times 2^frac_bits). While it is < 2^24, every
    partial sum of every layer, in every summation order, is a multiple of that bit below
    2^24 of them: exact in float32."""
    vals = _int_forward(layers, x)
    h = np.abs(np.asarray(x, np.float64) - (layers["front"][0] if layers["front"] is not None else 0))
    worst = float(np.abs(np.asarray(x, np.float64)).max())  # the front-end's own operands
    for d, (_, a) in zip(layers["dense"], vals):
        worst = max(worst, float((h @ np.abs(d["W"]).T.astype(np.float64) + np.abs(d["b"])).max()))
        h = np.abs(a).astype(np.float64)
    return worst * 2 ** frac_bits(layers)


def int_expected_layers(layers):
    """What the loader must lower the probe to: per layer (K, N, act code, alpha, beta)."""
    code = {None: (0, 0.0, 0.0), "Relu": (2, 0.0, 0.0), "LeakyRelu": (5, 0.5, 0.0), "Elu": (1, 1.0, 0.0),
            "Clip": (6,) + INT_ACTS["Clip"]}
    out = []
    for l, d in enumerate(layers["dense"]):
        a = code[d["act"]]
        if l == len(layers["dense"]) - 1 and layers["tail"] is not None:
            a = (6, layers["tail"][0], layers["tail"][1])  # a Clip right after the last Gemm: the head's activation
        out.append((d["W"].shape[1], d["W"].shape[0]) + a)
    return out


# ---------------------------------------------------------------------------------------
# activation probes

SELU_ALPHA, SELU_GAMMA = 1.67326319217681884765625, 1.05070102214813232421875

# (id, op, attributes); Clip's attributes are its bounds
ACT_OPS = [("elu", "Elu", {}), ("elu_a07", "Elu", {"alpha": 0.7}), ("relu", "Relu", {}), ("tanh", "Tanh", {}),
           ("sigmoid", "Sigmoid", {}), ("leaky", "LeakyRelu", {"alpha": 0.1}), ("clip", "Clip", {"min": -1.0, "max": 1.5}),
           ("selu", "Selu", {}), ("selu_attrs", "Selu", {"alpha": 1.2, "gamma": 0.8}), ("softplus", "Softplus", {}),
           ("hardsigmoid", "HardSigmoid", {"alpha": 0.3, "beta": 0.4}), ("hardswish", "HardSwish", {}),
           ("softsign", "Softsign", {})]
ACT_CODE = {"Elu": 1, "Relu": 2, "Tanh": 3, "Sigmoid": 4, "LeakyRelu": 5, "Clip": 6, "Selu": 7, "Softplus": 8,
            "HardSigmoid": 9, "HardSwish": 10, "Softsign": 11}

POINTS = [2.0 ** -100, 1e-30, 1e-8, 1e-6, 1e-4, 3e-4, 2.0 ** -10, 1e-3, 0.01, 0.1, 0.5, 1, 1.5, 2, 3, 5, 8, 10, 15, 17, 20,
          30, 50, 87, 88, 89, 100, 1e3, 1e4, 1e30]


def _f32(v):
    return float(np.float32(v))


def act_attrs(op, attrs):
    """(alpha, beta) as the loader holds them: the float32 attributes with the ONNX defaults."""
    if op == "Elu":
        return _f32(attrs.get("alpha", 1.0)), 0.0
    if op == "LeakyRelu":
        return _f32(attrs.get("alpha", 0.01)), 0.0
    if op == "Selu":
        return _f32(attrs.get("alpha", SELU_ALPHA)), _f32(attrs.get("gamma", SELU_GAMMA))
    if op == "HardSigmoid":
        return _f32(attrs.get("alpha", 0.2)), _f32(attrs.get("beta", 0.5))
    if op == "HardSwish":
        return _f32(1.0 / 6.0), 0.5
    if op == "Clip":
        return _f32(attrs["min"]), _f32(attrs["max"])
    return 0.0, 0.0


def act_points(op, attrs):
    """float32 points of the probe of `op`: +0, -0, +-POINTS and the op's own corners."""
    p = [0.0, -0.0]
    for v in POINTS:
        p += [v, -v]
    if op == "Clip":
        for b in (np.float32(attrs["min"]), np.float32(attrs["max"])):
            p += [b, np.nextafter(b, np.float32(-np.inf)), np.nextafter(b, np.float32(np.inf))]
    if op == "HardSigmoid":
        al, be = act_attrs(op, attrs)
        p += [-be / al, (1.0 - be) / al]
    return np.asarray(p, np.float32)


def act_inputs(points, in_dim, out_dim, rows=None):
    """The points packed out_dim per observation row (the rest of the row zero); rows: that
    many rows, the packed ones repeated in order. Returns (x [rows, in_dim] float32, the
    point of every output [rows, out_dim])."""
    n = -(-len(points) // out_dim)
    pts = np.zeros(n * out_dim, np.float32)
    pts[:len(points)] = points
    pts = pts.reshape(n, out_dim)
    if rows is not None:
        pts = pts[np.arange(rows) % n]
    x = np.zeros((pts.shape[0], in_dim), np.float32)
    x[:, :out_dim] = pts
    return x, pts


def act_eval(op, attrs, x):
    """The ONNX formula of `op` per element in float64 (numpy's IEEE semantics for +-inf)."""
    x = np.asarray(x, np.float64)
    al, be = act_attrs(op, attrs)
    with np.errstate(all="ignore"):
        if op == "Elu":
            return np.where(x > 0, x, al * np.expm1(np.minimum(x, 0)))
        if op == "Relu":
            return np.maximum(x, 0)
        if op == "Tanh":
            return np.tanh(x)
        if op == "Sigmoid":
            return 1.0 / (1.0 + np.exp(-x))
        if op == "LeakyRelu":
            return np.where(x >= 0, x, al * x)
        if op == "Clip":
            return np.minimum(np.maximum(x, al), be)
        if op == "Selu":
            return be * np.where(x > 0, x, al * np.expm1(np.minimum(x, 0)))
        if op == "Softplus":
            return np.log1p(np.exp(-np.abs(x))) + np.maximum(x, 0)
        if op == "HardSigmoid":
            return np.maximum(0, np.minimum(1, al * x + be))
        if op == "HardSwish":
            return x * np.maximum(0, np.minimum(1, x / 6.0 + 0.5))
        if op == "Softsign":
            return x / (1 + np.abs(x))
    raise KeyError(op)


def act_ref(op, attrs, pts, d=1):
    """act composed d times on the points, float64."""
    y = np.asarray(pts, np.float64)
    for _ in range(d):
        y = act_eval(op, attrs, y)
    return y


def act_bound(op, attrs, ref, d=1):
    """4 * 2^-23 * s * L_d * max(1, |ref|): s the op's scale (Elu max(1, |alpha|); Selu
    max(1, |alpha gamma|, |gamma|); else 1), L_d = sum_{i<d} Lip^i with Lip = s for Elu and
    Selu, 1.5 for HardSwish, 1 otherwise. 4 ulp: v_exp_f32, v_rcp_f32 and v_log_f32 at about
    1 ulp each (device_fn.hpp), one rounding for the argument's scale and one for the final
    add make about 2.5 for the worst op; the rest is margin for tanhf and for a contracted
    against an uncontracted multiply-add. Not a measurement of the kernels."""
    return 4.0 * 2.0 ** -23 * act_unit(op, attrs, d) * np.maximum(1.0, np.abs(ref))


def act_unit(op, attrs, d=1):
    """s * L_d of act_bound (the unit of the measured-error tables, times 2^-23 max(1, |ref|))."""
    al, be = act_attrs(op, attrs)
    s = max(1.0, abs(al)) if op == "Elu" else max(1.0, abs(al * be), abs(be)) if op == "Selu" else 1.0
    lip = s if op in ("Elu", "Selu") else 1.5 if op == "HardSwish" else 1.0
    return s * sum(lip ** i for i in range(d))


def act_policy(in_dim, hidden, out_dim, op, attrs, where, diag=1.0):
    """onnx bytes of in_dim -> hidden[0] -> ... -> out_dim: layer 0 is `diag` times the
    identity on the first in_dim units, further hidden layers are identities, the head
    selects the first out_dim units; all biases 0. where = "hidden": `op` after every hidden
    layer (d = len(hidden) compositions); "head": no hidden activation (Gemm -> Gemm), `op`
    after the last Gemm."""
    hidden = list(hidden)
    assert where in ("hidden", "head") and in_dim <= hidden[0] and out_dim <= min(in_dim, hidden[-1])
    dims = [in_dim] + hidden + [out_dim]
    nodes, inits, cur = [], [], "obs"
    for l, (K, N) in enumerate(zip(dims[:-1], dims[1:])):
        W = np.zeros((N, K), np.float32)
        i = np.arange(min(N, K))
        W[i, i] = diag if l == 0 else 1.0
        inits += [(f"W{l}", W), (f"b{l}", np.zeros(N, np.float32))]
        nodes.append(ow.node("Gemm", [cur, f"W{l}", f"b{l}"], [f"g{l}"], "", [ow.attr_int("transB", 1)]))
        cur = f"g{l}"
        last = l == len(dims) - 2
        if (where == "hidden") != last:
            if op == "Clip":
                inits += [(f"lo{l}", np.array(attrs["min"], np.float32)), (f"hi{l}", np.array(attrs["max"], np.float32))]
                nodes.append(ow.node("Clip", [cur, f"lo{l}", f"hi{l}"], [f"a{l}"]))
            else:
                nodes.append(ow.node(op, [cur], [f"a{l}"], "", [ow.attr_float(k, v) for k, v in attrs.items()]))
            cur = f"a{l}"
    nodes.append(ow.node("Identity", [cur], ["act"]))
    return ow.model(nodes, inits, [("obs", ["N", in_dim])], [("act", ["N", out_dim])])


OVERFLOW_ROWS = 8


def overflow_case(op, attrs, in_dim, hidden, out_dim):
    """(x [8, in_dim], ref [8, out_dim] float32) for act_policy(..., where="hidden", diag=2)
    with one hidden layer: row r holds 3e38 (even r) or -3e38 (odd r) in column r // 2, so that
    unit's pre-activation, the float32 product 2 x, is +-inf.
    The reference evaluates the activation in float64 on that float32 pre-activation and the
    head's identity select with IEEE semantics (0 * inf = NaN for the row's other outputs
    when act(+-inf) is not finite), cast to float32."""
    x = np.zeros((OVERFLOW_ROWS, in_dim), np.float32)
    for r in range(OVERFLOW_ROWS):
        x[r, (r // 2) % out_dim] = 3e38 if r % 2 == 0 else -3e38
    with np.errstate(all="ignore"):
        z = np.zeros((OVERFLOW_ROWS, hidden), np.float32)
        z[:, :in_dim] = np.float32(2.0) * x
        a = act_eval(op, attrs, z.astype(np.float64))
        head = np.zeros((out_dim, hidden), np.float64)
        head[np.arange(out_dim), np.arange(out_dim)] = 1.0
        y = np.stack([(head * a[r][None, :]).sum(1) for r in range(OVERFLOW_ROWS)])
    return x, y.astype(np.float32)


# ---------------------------------------------------------------------------------------
# the probes the CPU and GPU tests share: name -> int_policy arguments

def _p(dims, act, signed, front=False, tail=False):
    return dict(dims=tuple(dims), act=act, signed=signed, front=front, tail=tail)


NN, SR, SL = ("Elu", False), ("Relu", True), ("LeakyRelu", True)   # non-negative Elu, signed Relu, signed LeakyRelu 0.5

INT_PROBES = {
    # batch <= 8 forms (tests/test_gpu_probe_shapes.py SMALL)
    "33_1024_12": _p((33, 1024, 12), *NN),
    "33_1040_12": _p((33, 1040, 12), *SR),
    "20_512_40_9": _p((20, 512, 40, 9), *SL),
    "20_513_40_9": _p((20, 513, 40, 9), *NN),
    "16_4096_8": _p((16, 4096, 8), *NN),
    "16_4112_8": _p((16, 4112, 8), *NN),
    "24_64_16": _p((24, 64, 16), *SR),
    "24_64_17": _p((24, 64, 17), *NN),
    "1_64_3": _p((1, 64, 3), *NN),
    "3_64_3": _p((3, 64, 3), *SR),
    "63_128x2_12": _p((63, 128, 128, 12), *NN),
    "64_128x2_12": _p((64, 128, 128, 12), *SL),
    "65_128x2_12": _p((65, 128, 128, 12), "Clip", False),
    "48_64_12": _p((48, 64, 12), *SR),
    "98_128x2_12": _p((98, 128, 128, 12), *NN),
    "98_128x2_12_ft": _p((98, 128, 128, 12), *NN, front=True, tail=True),
    "200_64x3_12": _p((200, 64, 64, 64, 12), *SL),
    "150_128x2_12": _p((150, 128, 128, 12), *NN),
    "200_128x3_12": _p((200, 128, 128, 128, 12), *SR),
    "17_100_200_33_5": _p((17, 100, 200, 33, 5), *SR),
    "48_512x3_12": _p((48, 512, 512, 512, 12), *NN),
    "48_512x3_12_ft": _p((48, 512, 512, 512, 12), *NN, front=True, tail=True),
    "63_512x2_16": _p((63, 512, 512, 16), *SR),
    "17_256x2_1": _p((17, 256, 256, 1), *NN),
    "60_256x3_12": _p((60, 256, 256, 256, 12), *SL),
    # batched forms (BATCHED), those not above
    "30_96_160_64_200_9": _p((30, 96, 160, 64, 200, 9), *SR),
    "40_64_20": _p((40, 64, 20), *SR),
    "48_128_12_relu": _p((48, 128, 12), *SR),
    "64_128x2_20": _p((64, 128, 128, 20), *NN),
    "33_256x3_12": _p((33, 256, 256, 256, 12), *NN),
    "100_256x2_32": _p((100, 256, 256, 32), *SL),
    "48_512x3_12_relu": _p((48, 512, 512, 512, 12), *SR),
    "70_512_16": _p((70, 512, 16), *NN),
    "48_512x4_12": _p((48, 512, 512, 512, 512, 12), *NN),
}

_built = {}


def int_probe(name):
    """(onnx bytes, layers) of INT_PROBES[name], built once."""
    if name not in _built:
        _built[name] = int_policy(**INT_PROBES[name])
    return _built[name]


# the schedules each probe is run with on the GPU (tests/test_gpu_probe_shapes.py)
SMALL_PROBES = ["33_1024_12", "33_1040_12", "20_512_40_9", "20_513_40_9", "16_4096_8", "16_4112_8", "24_64_16", "24_64_17",
                "1_64_3", "3_64_3", "63_128x2_12", "64_128x2_12", "65_128x2_12", "48_64_12", "98_128x2_12",
                "98_128x2_12_ft", "200_64x3_12", "150_128x2_12", "200_128x3_12", "17_100_200_33_5", "48_512x3_12",
                "48_512x3_12_ft", "63_512x2_16", "17_256x2_1", "60_256x3_12"]
BATCHED_PROBES = ["17_100_200_33_5", "30_96_160_64_200_9", "40_64_20", "48_128_12_relu", "64_128x2_20", "33_256x3_12",
                  "100_256x2_32", "48_512x3_12", "48_512x3_12_relu", "70_512_16", "48_512x4_12", "98_128x2_12_ft",
                  "48_512x3_12_ft"]

# the activation probes' policies (tests/test_gpu_probe_activations.py): in, hidden, out
ACT_SHAPES = {"h64": (48, (64,), 12), "h128": (48, (128,), 12), "h128x3": (48, (128, 128, 128), 12),
              "h256x2": (48, (256, 256), 12)}


def run_checked(e, x):
    """e.run(x); a device error (a fault, not a wrong answer) ends the whole session, so that
    nothing more is started on a GPU that has just faulted."""
    import pytest
    from go2_onnx_controller_amd.engine import Go2piError
    try:
        return e.run(x)
    except Go2piError as ex:
        if ex.code == -3:
            pytest.exit(f"device error, stopping: {ex}", returncode=3)
        raise
