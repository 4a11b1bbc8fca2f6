"""CPU oracle for the seq2seq-LSTM hot path of ChengeLi/LongTerm360FoV.

TEST INFRASTRUCTURE ONLY.  Nothing under ``longterm360fov_amd/`` may import this module; only
``tests/``, ``__graft_entry__.smoke()`` and the ``cpu_baseline`` leg of ``bench.py`` do, and
only as the checker.  The product path is the HIP library behind ``include/fov360.h``.

PARITY STATUS
  * Data side (windowing, mu/sigma^2 features, clip): PINNED against the reference's own NumPy
    code, executed in the authoring container on seeded inputs
    (``tests/golden/make_data_fixtures.py`` -> ``tests/golden/data_helpers.npz``).
  * LSTM / Dense arithmetic: **parity unpinned**.  The reference delegates it to Keras 2.1-2.2
    on TensorFlow 1.x (``from keras.layers import LSTM, Dense`` - mycode/FoV_seq2seq.py:2-4),
    neither of which is present in /root/reference or installable here, and the reference holds
    no tests, golden vectors or trained weights for it.  This file
    restates the published Keras-2.2 ``LSTMCell`` / ``Dense`` definitions; the restatement is
    cross-checked against an independent implementation with the same gate order
    (``torch.nn.LSTM`` on CPU, sigmoid mode) and against hand-computed known-answer cases for
    ``hard_sigmoid`` in ``tests/test_oracle.py``.

Equations (Keras 2.2 ``LSTMCell.call``; kernel K:(F,4H), recurrent kernel R:(H,4H), bias b:(4H,),
gate column blocks in the order i, f, c, o):
    z   = x_t @ K + b + h_{t-1} @ R
    i   = s(z_i); f = s(z_f); o = s(z_o); g = tanh(z_c)
    c_t = f * c_{t-1} + i * g
    h_t = o * tanh(c_t)
with s = ``hard_sigmoid`` = clip(0.2 x + 0.5, 0, 1) (Keras < 2.3 default for
``recurrent_activation``; the reference never overrides it) or ``sigmoid`` (what
BASELINE.json's north_star names).  Both are implemented; callers choose with ``act``.
"""
import numpy as np

ACT_SIGMOID = 0
ACT_HARD_SIGMOID = 1
_ACT_NAMES = {"sigmoid": ACT_SIGMOID, "hard_sigmoid": ACT_HARD_SIGMOID,
              ACT_SIGMOID: ACT_SIGMOID, ACT_HARD_SIGMOID: ACT_HARD_SIGMOID}


def act_code(act):
    return _ACT_NAMES[act]


def sigmoid(x):
    # numerically stable logistic in the array's own dtype
    x = np.asarray(x)
    out = np.empty_like(x)
    pos = x >= 0
    out[pos] = 1 / (1 + np.exp(-x[pos]))
    e = np.exp(x[~pos])
    out[~pos] = e / (1 + e)
    return out


def hard_sigmoid(x):
    """Keras backend hard_sigmoid: clip(0.2*x + 0.5, 0, 1)."""
    x = np.asarray(x)
    return np.clip(x.dtype.type(0.2) * x + x.dtype.type(0.5), 0, 1).astype(x.dtype)


def _rec_act(act):
    return hard_sigmoid if act_code(act) == ACT_HARD_SIGMOID else sigmoid


# --------------------------------------------------------------------------------------
# a1/a2: Keras LSTM layer  (mycode/FoV_seq2seq.py:83-86, 93-95)
# --------------------------------------------------------------------------------------
# configs[4] (bf16): the HIP path feeds bf16 operands (round-to-nearest-even of the fp32 value) into the matrix cores
# and accumulates in fp32; cell state, gates and everything elementwise stay fp32.  `bf16_operands()` makes the
# matrix products of the LSTM steps and of the Dense(6) head below round BOTH operands the same way, so the
# restatement can be compared with the bf16 kernels far more tightly than the full-precision one.
OPERAND_ROUND = None


def round_bf16(a):
    """Round-to-nearest-even to bfloat16, returned in the input's dtype (what v_cvt_pk_bf16_f32 does to an fp32)."""
    a32 = np.ascontiguousarray(a, dtype=np.float32)
    u = a32.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32).reshape(a32.shape).astype(np.asarray(a).dtype)


class bf16_operands:
    """with bf16_operands(): ... -> matrix products of lstm_step / the Dense head see bf16-rounded operands."""

    def __enter__(self):
        global OPERAND_ROUND
        self._prev, OPERAND_ROUND = OPERAND_ROUND, round_bf16
        return self

    def __exit__(self, *exc):
        global OPERAND_ROUND
        OPERAND_ROUND = self._prev
        return False


def _mm(a, w):
    if OPERAND_ROUND is not None:
        a, w = OPERAND_ROUND(a), OPERAND_ROUND(w)
    return a @ w


def lstm_step(x, h, c, K, R, b, act="sigmoid"):
    """One LSTMCell step.  x:(B,F) h,c:(B,H) -> (h', c')."""
    H = h.shape[1]
    z = _mm(x, K) + b + _mm(h, R)
    s = _rec_act(act)
    i = s(z[:, 0 * H:1 * H])
    f = s(z[:, 1 * H:2 * H])
    g = np.tanh(z[:, 2 * H:3 * H])
    o = s(z[:, 3 * H:4 * H])
    c_new = f * c + i * g
    h_new = o * np.tanh(c_new)
    return h_new.astype(x.dtype), c_new.astype(x.dtype)


def lstm_layer(x, K, R, b, h0=None, c0=None, act="sigmoid"):
    """LSTM over x:(B,T,F).  Returns (hs:(B,T,H), h_T, c_T).  Zero initial state by default
    (Keras ``get_initial_state``); ``initial_state=[h, c]`` as in FoV_seq2seq.py:94-95."""
    B, T, _ = x.shape
    H = R.shape[0]
    h = np.zeros((B, H), x.dtype) if h0 is None else h0.astype(x.dtype)
    c = np.zeros((B, H), x.dtype) if c0 is None else c0.astype(x.dtype)
    hs = np.empty((B, T, H), x.dtype)
    for t in range(T):
        h, c = lstm_step(x[:, t], h, c, K, R, b, act)
        hs[:, t] = h
    return hs, h, c


# a3: Dense(num_decoder_tokens, activation='tanh')  (mycode/FoV_seq2seq.py:96-97)
def dense(x, W, b, activation="tanh", matrix_core=False):
    """matrix_core: this product runs on the matrix cores in the bf16 path (operands rounded under bf16_operands())."""
    y = (_mm(x, W) if matrix_core else x @ W) + b
    if activation == "tanh":
        y = np.tanh(y)
    return y.astype(x.dtype)


# --------------------------------------------------------------------------------------
# Target-only seq2seq  (mycode/FoV_seq2seq.py)
# weights: dict(enc_K, enc_R, enc_b, dec_K, dec_R, dec_b, dense_W, dense_b)
# --------------------------------------------------------------------------------------
def seq2seq_teacher_forced(enc_in, dec_in, w, act="sigmoid"):
    """Training-graph forward, FoV_seq2seq.py:82-101: decoder consumes GT inputs (B,T_out,6)."""
    _, h, c = lstm_layer(enc_in, w["enc_K"], w["enc_R"], w["enc_b"], act=act)
    hs, _, _ = lstm_layer(dec_in, w["dec_K"], w["dec_R"], w["dec_b"], h, c, act=act)
    B, T, H = hs.shape
    return dense(hs.reshape(B * T, H), w["dense_W"], w["dense_b"]).reshape(B, T, -1)


def seq2seq_decode(enc_in, dec_in0, w, T_out, act="sigmoid"):
    """Autoregressive inference, FoV_seq2seq.py:137-178 (batched; the reference runs batch 1):
    states = encoder(enc_in); target = dec_in0 (B,1,6);
    repeat T_out: y,h,c = decoder(target,h,c); y = dense(y); target = y."""
    _, h, c = lstm_layer(enc_in, w["enc_K"], w["enc_R"], w["enc_b"], act=act)
    y = dec_in0[:, 0].astype(enc_in.dtype)
    out = []
    for _ in range(T_out):
        h, c = lstm_step(y, h, c, w["dec_K"], w["dec_R"], w["dec_b"], act)
        y = dense(h, w["dense_W"], w["dense_b"])
        out.append(y)
    return np.stack(out, axis=1)


def onelayer_tar_seq2seq_forward(enc_in, dec_in0, w, T_out, act="sigmoid", decoder_no_init_state=True,
                                 add_residual_link=False, enc_last_out_as_dec_in=False, dense_activation="tanh",
                                 embed_frame_state_enc2dec=False, has_reconstruct_loss=False):
    """Unrolled no-teacher-forcing target-only model, FoV_seq2seq_no_teac_forc.py:37-149 (onelayer_tar_seq2seq):
    encoder LSTM (:42-44); decoder input = dec_in0 (B,1,O), or Dense(encoder output) when
    cfg.enc_last_out_as_dec_in (:75-78); step 0 of the decoder starts from ZERO state when the script's
    `decoder_no_init_state` is set (:29,98-99), later steps carry the decoder's own state (:118);
    y_t = Dense(h_t) [+ residual_dense(decoder input), cfg.add_residual_link, :103-107]; y_t is fed back (:115).
    cfg.embed_frame_state_enc2dec (:47-52): the encoder's final h and c each pass a Dense(latent_dim, tanh) before they
    seed the decoders (the decoder INPUT under enc_last_out_as_dec_in still comes from the raw encoder output, :78).
    cfg.has_reconstruct_loss (:56-59,90-95,120-126): a second self-fed LSTM + Dense(num_encoder_tokens, tanh), seeded with
    the same (embedded) states and fed Dense_recons(encoder output) first, emits T_out reconstructed input seconds;
    the function then returns (prediction, reconstruction).
    weights: enc_*, dec_*, dense_W/b; res_W (O,O) / res_b; emb1_W/b, emb2_W/b (H,H); rec_K/R/b, recd_W (H,F) / recd_b."""
    fa = (lambda v: np.tanh(v)) if dense_activation == "tanh" else (lambda v: np.maximum(v, 0))
    _, h_enc, c_enc = lstm_layer(enc_in, w["enc_K"], w["enc_R"], w["enc_b"], act=act)
    sh, sc = h_enc, c_enc
    if embed_frame_state_enc2dec:
        sh = np.tanh(h_enc @ w["emb1_W"] + w["emb1_b"])
        sc = np.tanh(c_enc @ w["emb2_W"] + w["emb2_b"])
    if enc_last_out_as_dec_in:
        x0 = fa(h_enc @ w["dense_W"] + w["dense_b"])
    else:
        x0 = dec_in0[:, 0].astype(enc_in.dtype)
    h, c = (np.zeros_like(sh), np.zeros_like(sc)) if decoder_no_init_state else (sh, sc)
    r = fa(x0 @ w["res_W"] + w["res_b"]) if add_residual_link else 0.0
    x, out = x0, []
    for _ in range(T_out):
        h, c = lstm_step(x, h, c, w["dec_K"], w["dec_R"], w["dec_b"], act)
        x = fa(h @ w["dense_W"] + w["dense_b"]) + r
        out.append(x)
    y = np.stack(out, axis=1)
    if not has_reconstruct_loss:
        return y
    x, h, c, rec = np.tanh(h_enc @ w["recd_W"] + w["recd_b"]), sh, sc, []
    for _ in range(T_out):
        h, c = lstm_step(x, h, c, w["rec_K"], w["rec_R"], w["rec_b"], act)
        x = np.tanh(h @ w["recd_W"] + w["recd_b"])
        rec.append(x)
    return y, np.stack(rec, axis=1)


def stacked_seq2seq_forward(enc_in, dec_in, w, num_layers, act="sigmoid", T_out=None):
    """L-layer target-only seq2seq, Fov_seq2seq_2layers.py:232-272 / 3layers.py:222-277.  weights enc{l}_K/R/b, dec{l}_K/R/b,
    dense_W/b.  T_out None: teacher-forced graph on dec_in (B,T_out,O).  T_out given: the autoregressive loop of
    :399-430 from dec_in (B,1,O), each Dense output fed back."""
    states, inp = [], enc_in
    for l in range(num_layers):
        inp, h, c = lstm_layer(inp, w["enc%d_K" % l], w["enc%d_R" % l], w["enc%d_b" % l], act=act)
        states.append([h, c])
    if T_out is None:
        inp = dec_in
        for l in range(num_layers):
            inp, _, _ = lstm_layer(inp, w["dec%d_K" % l], w["dec%d_R" % l], w["dec%d_b" % l], states[l][0], states[l][1], act=act)
        return dense(inp, w["dense_W"], w["dense_b"])
    x, out = dec_in[:, 0].astype(enc_in.dtype), []
    for _ in range(T_out):
        for l in range(num_layers):
            states[l] = list(lstm_step(x, states[l][0], states[l][1], w["dec%d_K" % l], w["dec%d_R" % l], w["dec%d_b" % l], act))
            x = states[l][0]
        x = dense(x, w["dense_W"], w["dense_b"])
        out.append(x)
    return np.stack(out, axis=1)


def single_lstm_keras_forward(x, w, T_out=None, unrolled=False, noise=None, act="sigmoid"):
    """mycode/lstm_keras.py, weights K, R, b, dense_W, dense_b.  unrolled False: 1st part (:70-80), one input second per
    step from zero state, Dense(6,tanh) on every h.  unrolled True: the sampling model / 2nd part (:131-153,218-240) on
    ONE input second (B,1,F); noise None: `this_inputs` is never replaced, the same second feeds every step; noise
    (T_out-1,B,3*fps): cfg.predict_mean_var and cfg.sample_and_refeed - the next input is
    [N(mu_x, var_x) * fps | N(mu_y, var_y) * fps | N(mu_z, var_z) * fps] with the predicted VARIANCE used as stddev
    (:39-44) = mu + var * noise in that planar layout (:147-149)."""
    if not unrolled:
        hs, _, _ = lstm_layer(x, w["K"], w["R"], w["b"], act=act)
        return dense(hs, w["dense_W"], w["dense_b"])
    B, F = x.shape[0], x.shape[2]
    fps = F // 3
    H = w["R"].shape[0]
    h, c = np.zeros((B, H), x.dtype), np.zeros((B, H), x.dtype)
    xin, out = x[:, 0], []
    for t in range(T_out):
        h, c = lstm_step(xin, h, c, w["K"], w["R"], w["b"], act)
        y = dense(h, w["dense_W"], w["dense_b"])
        out.append(y)
        if noise is not None and t < T_out - 1:
            xin = (y[:, :3, None] + y[:, 3:6, None] * noise[t].reshape(B, 3, fps)).reshape(B, F)
    return np.stack(out, axis=1)


# --------------------------------------------------------------------------------------
# a4: target + others mixing, 2-layer, no teacher forcing
# (mycode/given_others_gt_mean_var_seq2seq.py:98-130, 203-299)
# weights: enc1_*, enc2_*, dec1_*, dec2_*, dense_W/b (H,6), mix_W (6*U,6), mix_b
# --------------------------------------------------------------------------------------
def others_mixing_forward(enc_in, others, dec_in0, w, act="sigmoid", mixing="mlp"):
    """enc_in:(B,T_in,F) others:(B,T_out,U-1,6) dec_in0:(B,1,6) -> (B,T_out,6).
    Per step: d1=LSTM1(x); d2=LSTM2(d1); p=tanh(d2 Wd+bd);
    mixing 'mlp' (mlp_mixing, :166-168,262-265): m=tanh(flatten(concat_axis1[others[:,t], p]) Wm + bm) (user-major flatten,
    pred last); mixing 'conv' (conv_mixing, :188-197,284-290): the (U,6) stack is permuted to a 1x6 map with the U users
    as channels and passes three Conv2D(1x3, same, relu) layers with 8, 8 and 1 filters (weights mixc{0,1,2}_W (1,3,C,N),
    mixc{0,1,2}_b); the single output channel is m.  x=m is fed back."""
    hs1, h1, c1 = lstm_layer(enc_in, w["enc1_K"], w["enc1_R"], w["enc1_b"], act=act)
    _, h2, c2 = lstm_layer(hs1, w["enc2_K"], w["enc2_R"], w["enc2_b"], act=act)
    x = dec_in0[:, 0].astype(enc_in.dtype)
    B, T_out = others.shape[0], others.shape[1]
    out = []
    for t in range(T_out):
        h1, c1 = lstm_step(x, h1, c1, w["dec1_K"], w["dec1_R"], w["dec1_b"], act)
        h2, c2 = lstm_step(h1, h2, c2, w["dec2_K"], w["dec2_R"], w["dec2_b"], act)
        p = dense(h2, w["dense_W"], w["dense_b"], matrix_core=True)    # (B,6)
        cat = np.concatenate([others[:, t].astype(x.dtype), p[:, None, :]], axis=1)  # (B,U,6)
        if mixing == "conv":
            a = np.transpose(cat, (0, 2, 1))[:, None]                   # Permute((2,1)) + expand_dims(1): (B,1,6,U)
            for i in range(3):
                a = np.maximum(conv2d_same(a, w["mixc%d_W" % i], w["mixc%d_b" % i]), 0)
            x = a[:, 0, :, 0]                                           # get_dim1 + Permute((2,1)): (B,6)
        else:
            x = dense(cat.reshape(B, -1), w["mix_W"], w["mix_b"])       # (B,6)
        out.append(x)
    return np.stack(out, axis=1)


def bidirectional_lstm(x, wf, wb, init=None, act="sigmoid"):
    """Keras Bidirectional(LSTM(return_sequences, return_state), merge_mode='concat'): the backward layer reads the
    sequence reversed and its outputs are reversed back before the concat.  wf / wb = (K, R, b); init = (fh, fc, bh, bc) or
    None.  -> (seq (B,T,2H), fh, fc, bh, bc)."""
    i = (None,) * 4 if init is None else init
    f_seq, fh, fc = lstm_layer(x, wf[0], wf[1], wf[2], i[0], i[1], act=act)
    b_seq, bh, bc = lstm_layer(x[:, ::-1], wb[0], wb[1], wb[2], i[2], i[3], act=act)
    return np.concatenate([f_seq, b_seq[:, ::-1]], axis=-1), fh, fc, bh, bc


def others_context_forward(enc_in, others, dec_in0, w, T_out, mode, act="sigmoid"):
    """The other decoder heads of given_others_gt_mean_var_seq2seq.py (2+2-layer model, no teacher forcing, :203-299):
      'target_user_only' (:219-220)  y_t = decoder_dense(h2_t)
      'others_mlp'       (:153-156,223-233)  ctx_t = relu(relu(flatten(others_t) W1 + b1) W2 + b2);  y_t = decoder_dense([ctx_t ; h2_t])
      'others_lstm'      (:157-166,234-240)  ctx = BiLSTM2(BiLSTM1(others reshaped (B,T,(U-1)*6))): calling the second
                         Bidirectional on the LIST the first returns makes layer 1's final states its initial states;
                         y_t = decoder_dense([ctx_t (2H) ; h2_t])
    y_t is fed back as the next decoder input.  weights: enc1/enc2/dec1/dec2 _K/_R/_b, dense_W ((Cc+H),6), dense_b, and
    oth_W1/b1/W2/b2 or ol{1,2}{f,b}_K/_R/_b."""
    hs1, h1, c1 = lstm_layer(enc_in, w["enc1_K"], w["enc1_R"], w["enc1_b"], act=act)
    _, h2, c2 = lstm_layer(hs1, w["enc2_K"], w["enc2_R"], w["enc2_b"], act=act)
    B = enc_in.shape[0]
    ctx = None
    if mode == "others_mlp":
        o = others.reshape(B, T_out, -1).astype(enc_in.dtype)
        ctx = np.maximum(np.maximum(o @ w["oth_W1"] + w["oth_b1"], 0) @ w["oth_W2"] + w["oth_b2"], 0)
    elif mode == "others_lstm":
        o = others.reshape(B, T_out, -1).astype(enc_in.dtype)
        g = lambda n: (w[n + "_K"], w[n + "_R"], w[n + "_b"])
        s1, fh, fc, bh, bc = bidirectional_lstm(o, g("ol1f"), g("ol1b"), act=act)
        ctx = bidirectional_lstm(s1, g("ol2f"), g("ol2b"), (fh, fc, bh, bc), act=act)[0]
    x, out = dec_in0[:, 0].astype(enc_in.dtype), []
    for t in range(T_out):
        h1, c1 = lstm_step(x, h1, c1, w["dec1_K"], w["dec1_R"], w["dec1_b"], act)
        h2, c2 = lstm_step(h1, h2, c2, w["dec2_K"], w["dec2_R"], w["dec2_b"], act)
        x = dense(h2 if ctx is None else np.concatenate([ctx[:, t], h2], axis=1), w["dense_W"], w["dense_b"])
        out.append(x)
    return np.stack(out, axis=1)


# --------------------------------------------------------------------------------------
# a5: mu / sigma^2 features  (mycode/utility.py:483-517)
# --------------------------------------------------------------------------------------
def meanvar_xyz(y):
    """(N,T,90) interleaved xyzxyz.. or (N,T,30,3) -> (N,T,6) = [mx,my,mz,vx,vy,vz]; ddof=0.
    Slices per axis exactly as utility.py:484-499 does, so float64 results are bit-identical."""
    if y.shape[-1] == 3:
        assert y.ndim == 4
        comps = [y[:, :, :, a] for a in range(3)]
    else:
        assert y.ndim == 3 and y.shape[-1] % 3 == 0
        comps = [y[:, :, a::3] for a in range(3)]
    means = [np.mean(c, axis=-1)[:, :, np.newaxis] for c in comps]
    variances = [np.var(c, axis=-1)[:, :, np.newaxis] for c in comps]
    return np.concatenate(means + variances, axis=-1)


def meanvar_xyz_oth(y):
    """(N,T,U,30,3) -> (N,T,U,6)   (utility.py:505-517)."""
    assert y.ndim == 5 and y.shape[-1] == 3
    comps = [y[:, :, :, :, a] for a in range(3)]
    means = [np.mean(c, axis=-1)[:, :, :, np.newaxis] for c in comps]
    variances = [np.var(c, axis=-1)[:, :, :, np.newaxis] for c in comps]
    return np.concatenate(means + variances, axis=-1)


# a6: Keras mean_squared_error + sample mean  (mycode/cost.py:20-22)
def mse(y_true, y_pred):
    return float(np.mean(np.mean((y_pred.astype(np.float64) - y_true.astype(np.float64)) ** 2, axis=-1)))


# --------------------------------------------------------------------------------------
# Keras default initialisers (glorot_uniform kernel, orthogonal recurrent, unit_forget_bias)
# --------------------------------------------------------------------------------------
def _glorot_uniform(rng, fan_in, fan_out, dtype):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, (fan_in, fan_out)).astype(dtype)


def _orthogonal(rng, rows, cols, dtype):
    a = rng.standard_normal((rows, cols))
    u, _, vt = np.linalg.svd(a, full_matrices=False)
    q = u if u.shape == (rows, cols) else vt
    return q.astype(dtype)


def init_lstm(rng, F, H, dtype=np.float32):
    K = _glorot_uniform(rng, F, 4 * H, dtype)
    R = _orthogonal(rng, H, 4 * H, dtype)
    b = np.zeros(4 * H, dtype)
    b[H:2 * H] = 1  # unit_forget_bias
    return K, R, b


def init_seq2seq(seed, F_enc=90, F_dec=6, H=256, dtype=np.float32, bias_noise=0.0):
    rng = np.random.default_rng(seed)
    w = {}
    w["enc_K"], w["enc_R"], w["enc_b"] = init_lstm(rng, F_enc, H, dtype)
    w["dec_K"], w["dec_R"], w["dec_b"] = init_lstm(rng, F_dec, H, dtype)
    w["dense_W"] = _glorot_uniform(rng, H, F_dec, dtype)
    w["dense_b"] = np.zeros(F_dec, dtype)
    if bias_noise:
        for k in ("enc_b", "dec_b", "dense_b"):
            w[k] = (w[k] + bias_noise * rng.standard_normal(w[k].shape)).astype(dtype)
    return w


def init_others_mixing(seed, F_enc=90, F_dec=6, H=256, num_user=34, dtype=np.float32, bias_noise=0.0):
    rng = np.random.default_rng(seed)
    w = {}
    for name, F in (("enc1", F_enc), ("enc2", H), ("dec1", F_dec), ("dec2", H)):
        w[name + "_K"], w[name + "_R"], w[name + "_b"] = init_lstm(rng, F, H, dtype)
    w["dense_W"] = _glorot_uniform(rng, H, F_dec, dtype)
    w["dense_b"] = np.zeros(F_dec, dtype)
    w["mix_W"] = _glorot_uniform(rng, num_user * F_dec, F_dec, dtype)
    w["mix_b"] = np.zeros(F_dec, dtype)
    if bias_noise:
        for k in list(w):
            if k.endswith("_b"):
                w[k] = (w[k] + bias_noise * rng.standard_normal(w[k].shape)).astype(dtype)
    return w


# --------------------------------------------------------------------------------------
# Synthetic trajectories of SURVEY.md section 8(d)
# --------------------------------------------------------------------------------------
def synthetic_xyz(rng, B, T, fps=30, dtype=np.float32):
    """(B, T, 3*fps) interleaved xyz per frame, smooth unit-sphere trajectories."""
    n = T * fps
    yaw = rng.uniform(-np.pi, np.pi, (B, 1)) + np.cumsum(rng.normal(0, 0.02, (B, n)), axis=1)
    pitch = np.clip(rng.normal(0, 0.3, (B, 1)) + np.cumsum(rng.normal(0, 0.01, (B, n)), axis=1), -np.pi / 2, np.pi / 2)
    xyz = np.stack([np.cos(pitch) * np.cos(yaw), np.cos(pitch) * np.sin(yaw), np.sin(pitch)], axis=-1)
    return xyz.reshape(B, T, fps * 3).astype(dtype)


def synthetic_batch(seed, B, T_in, T_out, num_others=0, fps=30, dtype=np.float32):
    """enc_in (B,T_in,90), dec_in0 (B,1,6), target (B,T_out,6) [, others (B,T_out,U-1,6)]."""
    rng = np.random.default_rng(seed)
    traj = synthetic_xyz(rng, B, T_in + T_out, fps, np.float64)
    enc_in = traj[:, :T_in]
    target = meanvar_xyz(traj[:, T_in:])
    dec_in0 = meanvar_xyz(enc_in[:, -1:])
    out = [enc_in.astype(dtype), dec_in0.astype(dtype), target.astype(dtype)]
    if num_others:
        oth = synthetic_xyz(rng, B * num_others, T_out, fps, np.float64).reshape(B, num_others, T_out, fps, 3)
        out.append(meanvar_xyz_oth(oth.transpose(0, 2, 1, 3, 4)).astype(dtype))
    return tuple(out)


# --------------------------------------------------------------------------------------
# a6: training-graph backward (BPTT) and the Keras optimizers
# model.compile(optimizer='Adam', loss='mean_squared_error') - mycode/FoV_seq2seq.py:103
# The arithmetic is Keras/TensorFlow autodiff in the reference; this is the closed-form
# restatement, checked against torch.autograd and finite differences in tests/test_oracle.py.
# --------------------------------------------------------------------------------------
def _rec_act_grad(a, act):
    """d s(z)/dz expressed through the activation value a = s(z)."""
    if act_code(act) == ACT_HARD_SIGMOID:
        return np.where((a > 0) & (a < 1), a.dtype.type(0.2), a.dtype.type(0))
    return a * (1 - a)


def _rb_if(flag):
    """The operand map of a product: round_bf16 when its rounding switch is on, else the identity."""
    return round_bf16 if flag else (lambda a: a)


def lstm_layer_train(x, K, R, b, h0=None, c0=None, act="sigmoid", round_fwd=False):
    """Forward that also returns the reserve (i,f,g,o,c per step) the backward needs.  round_fwd: both products of every
    step take bf16-rounded operands (the bf16 forward kernels); off, the arithmetic is exactly the unrounded one."""
    B, T, _ = x.shape
    H = R.shape[0]
    h = np.zeros((B, H), x.dtype) if h0 is None else h0.astype(x.dtype)
    c = np.zeros((B, H), x.dtype) if c0 is None else c0.astype(x.dtype)
    s = _rec_act(act)
    hs = np.empty((B, T, H), x.dtype)
    res = np.empty((B, T, 5, H), x.dtype)
    if round_fwd:
        Kr, Rr = round_bf16(K), round_bf16(R)
    for t in range(T):
        if round_fwd:
            z = round_bf16(x[:, t]) @ Kr + b + round_bf16(h) @ Rr
        else:
            z = x[:, t] @ K + b + h @ R
        i, f, g, o = s(z[:, :H]), s(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), s(z[:, 3 * H:])
        c = f * c + i * g
        h = o * np.tanh(c)
        hs[:, t] = h
        res[:, t, 0], res[:, t, 1], res[:, t, 2], res[:, t, 3], res[:, t, 4] = i, f, g, o, c
    return hs, h, c, res


def lstm_layer_backward(x, K, R, h0, c0, hs, res, dhs=None, dhT=None, dcT=None, act="sigmoid", round_rec=False,
                        round_dx=False, round_wgrad=False):
    """BPTT of one LSTM layer.  Returns dict(dx, dK, dR, db, dh0, dc0, dz).
    Rounding switches (the bf16 backward kernels, see include/fov360.h): round_rec - the recurrence dh_{t-1} = dz_t R^T takes
    bf16-rounded operands; round_dx - the data gradient dx = dz K^T does; round_wgrad - the weight products x^T dz and
    h_{t-1}^T dz do.  db is always the sum of the unrounded dz, and dz itself is never rounded.  All off: the unrounded
    arithmetic, bit for bit."""
    B, T, F = x.shape
    H = R.shape[0]
    dt = x.dtype
    h0 = np.zeros((B, H), dt) if h0 is None else h0
    c0 = np.zeros((B, H), dt) if c0 is None else c0
    dh = np.zeros((B, H), dt) if dhT is None else dhT.astype(dt).copy()
    dc = np.zeros((B, H), dt) if dcT is None else dcT.astype(dt).copy()
    dz_all = np.empty((B, T, 4 * H), dt)
    if round_rec:
        RrT = round_bf16(R).T
    for t in range(T - 1, -1, -1):
        i, f, g, o, c = (res[:, t, q] for q in range(5))
        c_prev = res[:, t - 1, 4] if t > 0 else c0
        if dhs is not None:
            dh = dh + dhs[:, t]
        tc = np.tanh(c)
        do = dh * tc
        dc = dc + dh * o * (1 - tc * tc)
        dz = np.concatenate([dc * g * _rec_act_grad(i, act), dc * c_prev * _rec_act_grad(f, act),
                             dc * i * (1 - g * g), do * _rec_act_grad(o, act)], axis=1)
        dz_all[:, t] = dz
        dc = dc * f
        dh = round_bf16(dz) @ RrT if round_rec else dz @ R.T
    hprev = np.concatenate([h0[:, None], hs[:, :-1]], axis=1)
    dz2 = dz_all.reshape(B * T, 4 * H)
    rx, rw = _rb_if(round_dx), _rb_if(round_wgrad)
    return {"dx": (rx(dz2) @ rx(K).T).reshape(B, T, F), "dK": rw(x.reshape(B * T, F)).T @ rw(dz2),
            "dR": rw(hprev.reshape(B * T, H)).T @ rw(dz2), "db": dz2.sum(axis=0), "dh0": dh, "dc0": dc, "dz": dz_all}


# --------------------------------------------------------------------------------------
# The unrolled others-mixing decoder of the a4 training graph (given_others_gt_mean_var_seq2seq.py:203-308) as the fused
# decoder kernels see it: inputs are the encoder's final states, the decoder's first input dec0 (B,O) and the others'
# projection oth_proj (B,T,O) = others_t . mix_W[others' rows] + mix_b.  Per step t (x_0 = dec0, x_{t+1} = m_t):
#     h1, c1 = LSTM1(x_t, h1, c1);  h2, c2 = LSTM2(h1, h2, c2);  p_t = tanh(h2 dense_W + dense_b);
#     m_t = tanh(p_t mix_Wp + oth_proj_t)                  (mix_Wp = the prediction's (O,O) rows of mix_W)
# Tapes, time-major like ops.mix_decoder(train=...): P, M (T,B,O); H1, C1, H2, C2 (T,B,H) = states AFTER step t;
# res1, res2 (T,B,5,H) = activated i, f, g, o and c of step t.
# --------------------------------------------------------------------------------------
def mix_decoder_train_forward(dec0, h1, c1, h2, c2, oth_proj, w, mix_Wp, T_out, act="sigmoid", round_fwd=False):
    """round_fwd: the two gate products of each layer and the Dense head's product take bf16-rounded operands (the bf16
    decoder kernel); the mixing product p mix_Wp stays unrounded.  -> dict(M, P, H1, C1, H2, C2, res1, res2)."""
    s = _rec_act(act)
    r = _rb_if(round_fwd)
    K1, R1, K2, R2, Wd = (r(w[k]) for k in ("dec1_K", "dec1_R", "dec2_K", "dec2_R", "dense_W"))
    B, H = h1.shape
    x = dec0.reshape(B, -1)
    tape = {k: [] for k in ("M", "P", "H1", "C1", "H2", "C2", "res1", "res2")}

    def step(x, h, c, K, R, b):
        z = r(x) @ K + b + r(h) @ R
        i, f, g, o = s(z[:, :H]), s(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), s(z[:, 3 * H:])
        c = f * c + i * g
        return o * np.tanh(c), c, np.stack([i, f, g, o, c], axis=1)

    for t in range(T_out):
        h1, c1, q1 = step(x, h1, c1, K1, R1, w["dec1_b"])
        h2, c2, q2 = step(h1, h2, c2, K2, R2, w["dec2_b"])
        p = np.tanh(r(h2) @ Wd + w["dense_b"])
        x = np.tanh(p @ mix_Wp + oth_proj[:, t])
        for k, v in (("M", x), ("P", p), ("H1", h1), ("C1", c1), ("H2", h2), ("C2", c2), ("res1", q1), ("res2", q2)):
            tape[k].append(v)
    return {k: np.stack(v) for k, v in tape.items()}


def mix_decoder_backward(M, P, dloss, res1, res2, C1, C2, w, mix_Wp, act="sigmoid", round_rec=False, round_dx=False):
    """BPTT through the unrolled decoder from the fused kernels' own tapes: what ops.mix_decoder_bwd returns.
    M, P, dloss (T,B,O) - dloss = dL/d(pre-tanh of m_t) from the loss alone; res1, res2 (T,B,5,H); C1, C2: >= T rows of
    (B,H), row t = the cell state BEFORE step t.  The feedback x_{t+1} = m_t adds dx_{t+1} (1 - m_t^2) to dpre_m of step t.
    round_rec: the recurrences dz2 R2^T and dz1 R1^T take bf16-rounded operands; round_dx: the data-gradient products
    dz2 K2^T (-> dh1_t) and dz1 K1^T (-> dx_t, the feedback) do.  The head (dpre_m mix_Wp^T, dpre_p dense_W^T) is unrounded.
    -> dict(DZ1, DZ2 (T,B,4H), dpre_m, dpre_p (T,B,O), dh1_0, dc1_0, dh2_0, dc2_0 (B,H))."""
    T, B, O = M.shape
    H = w["dec1_R"].shape[0]
    ar, ax = _rb_if(round_rec), _rb_if(round_dx)
    R1T, R2T, K1T, K2T = ar(w["dec1_R"]).T, ar(w["dec2_R"]).T, ax(w["dec1_K"]).T, ax(w["dec2_K"]).T
    dt = M.dtype
    dh1, dc1, dh2, dc2 = (np.zeros((B, H), dt) for _ in range(4))
    dx = np.zeros((B, O), dt)
    out = {"DZ1": np.empty((T, B, 4 * H), dt), "DZ2": np.empty((T, B, 4 * H), dt),
           "dpre_m": np.empty((T, B, O), dt), "dpre_p": np.empty((T, B, O), dt)}

    def gates(q, c_prev, dh, dc):
        i, f, g, o, c = (q[:, k] for k in range(5))
        tc = np.tanh(c)
        dc = dc + dh * o * (1 - tc * tc)
        dz = np.concatenate([dc * g * _rec_act_grad(i, act), dc * c_prev * _rec_act_grad(f, act),
                             dc * i * (1 - g * g), dh * tc * _rec_act_grad(o, act)], axis=1)
        return dz, dc * f

    for t in range(T - 1, -1, -1):
        dm = dloss[t] + dx * (1 - M[t] * M[t])
        dpp = (dm @ mix_Wp.T) * (1 - P[t] * P[t])
        dz2, dc2 = gates(res2[t], C2[t], dpp @ w["dense_W"].T + dh2, dc2)
        dh2 = ar(dz2) @ R2T
        dz1, dc1 = gates(res1[t], C1[t], ax(dz2) @ K2T + dh1, dc1)
        dh1 = ar(dz1) @ R1T
        dx = ax(dz1) @ K1T
        out["dpre_m"][t], out["dpre_p"][t], out["DZ2"][t], out["DZ1"][t] = dm, dpp, dz2, dz1
    out.update(dh1_0=dh1, dc1_0=dc1, dh2_0=dh2, dc2_0=dc2)
    return out


def seq2seq_loss_and_grads(enc_in, dec_in, target, w, act="sigmoid"):
    """Teacher-forced graph (FoV_seq2seq.py:82-103): loss = Keras mean_squared_error averaged over
    every sample and step; returns (loss, grads dict keyed like the weights, prediction)."""
    ehs, eh, ec, eres = lstm_layer_train(enc_in, w["enc_K"], w["enc_R"], w["enc_b"], act=act)
    dhs_, _, _, dres = lstm_layer_train(dec_in, w["dec_K"], w["dec_R"], w["dec_b"], eh, ec, act=act)
    B, T, H = dhs_.shape
    y = np.tanh(dhs_.reshape(B * T, H) @ w["dense_W"] + w["dense_b"])
    t2 = target.reshape(B * T, -1)
    loss = float(np.mean((y - t2) ** 2))
    dy = 2 * (y - t2) / y.size
    dpre = dy * (1 - y * y)
    g = {"dense_W": dhs_.reshape(B * T, H).T @ dpre, "dense_b": dpre.sum(axis=0)}
    d_dec_hs = (dpre @ w["dense_W"].T).reshape(B, T, H)
    bd = lstm_layer_backward(dec_in, w["dec_K"], w["dec_R"], eh, ec, dhs_, dres, dhs=d_dec_hs, act=act)
    g["dec_K"], g["dec_R"], g["dec_b"] = bd["dK"], bd["dR"], bd["db"]
    be = lstm_layer_backward(enc_in, w["enc_K"], w["enc_R"], None, None, ehs, eres, dhT=bd["dh0"], dcT=bd["dc0"], act=act)
    g["enc_K"], g["enc_R"], g["enc_b"] = be["dK"], be["dR"], be["db"]
    return loss, g, y.reshape(B, T, -1)


def adam_step(p, g, m, v, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7):
    """Keras-2.2 Adam.get_updates: lr_t = lr*sqrt(1-b2^t)/(1-b1^t); p -= lr_t * m / (sqrt(v) + eps).
    `t` is the 1-based step count.  In place on (p, m, v)."""
    lr_t = lr * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)
    m[...] = beta1 * m + (1 - beta1) * g
    v[...] = beta2 * v + (1 - beta2) * g * g
    p[...] = p - lr_t * m / (np.sqrt(v) + eps)


def rmsprop_step(p, g, a, lr=1e-3, rho=0.9, eps=1e-7):
    """Keras-2.2 RMSprop: a = rho*a + (1-rho)*g^2; p -= lr * g / (sqrt(a) + eps).  In place."""
    a[...] = rho * a + (1 - rho) * g * g
    p[...] = p - lr * g / (np.sqrt(a) + eps)


# --------------------------------------------------------------------------------------
# Loss / optimizer / pointwise references of tests/test_gpu_loss_optim_edges.py.  Every one is fp64 arithmetic ON THE
# fp32-ROUNDED inputs and hyper-parameters (r32): the kernels form 1.f - beta in fp32, and 1 - float32(0.999) is 1.3e-5 away
# from 1 - 0.999.  Next to each result comes the sum of the |terms| that make up each element, the weight of the
# per-element bound  |err| <= c * 2^-24 * weight  (a max|ref| scale would hide an error in an ordinary element).
# --------------------------------------------------------------------------------------
U24 = 2.0 ** -24


def r32(x):
    """The fp64 value of x after rounding to fp32 (what a kernel's float argument holds)."""
    return float(np.float32(x))


def _d(a):
    return np.asarray(a, dtype=np.float64)


def adam_lr_t(t, lr=1e-3, beta1=0.9, beta2=0.999):
    """The step size the library hands its Adam kernels: double arithmetic on the float arguments, rounded to float."""
    return r32(r32(lr) * np.sqrt(1.0 - r32(beta2) ** t) / (1.0 - r32(beta1) ** t))


def adam_step_f32args(p, g, m, v, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, exact_betas=False):
    """One Adam step in fp64 from fp32 state with fp32-rounded hyper-parameters -> (p, m, v) and the weights of their bounds
    (p: |p| + |update|, m / v: their |terms|, upd: |update|, upd_m: what an error of m of one weight does to the update).
    exact_betas: the plain fp64 hyper-parameters instead (the reference the tests must be able to tell apart)."""
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    if exact_betas:
        b1, b2, e = beta1, beta2, eps
        lr_t = lr * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)
    else:
        b1, b2, e, lr_t = r32(beta1), r32(beta2), r32(eps), adam_lr_t(t, lr, beta1, beta2)
    mn = b1 * m + (1 - b1) * g
    vn = b2 * v + (1 - b2) * g * g
    den = np.sqrt(vn) + e
    upd = lr_t * mn / den
    wm = np.abs(b1 * m) + np.abs((1 - b1) * g)
    return (p - upd, mn, vn), {"p": np.abs(p) + np.abs(upd), "m": wm, "v": vn, "upd": np.abs(upd), "upd_m": lr_t * wm / den}


def rmsprop_step_f32args(p, g, a, lr=1e-3, rho=0.9, eps=1e-7):
    """Keras RMSprop, as adam_step_f32args -> (p, a), weights p / a / upd."""
    p, g, a = _d(p), _d(g), _d(a)
    lr, rho, eps = r32(lr), r32(rho), r32(eps)
    an = rho * a + (1 - rho) * g * g
    upd = lr * g / (np.sqrt(an) + eps)
    return (p - upd, an), {"p": np.abs(p) + np.abs(upd), "a": an, "upd": np.abs(upd)}


def rmsprop_tf_step(p, g, ms, lr, decay=0.9, eps=1e-10, clip=0.0):
    """tf.train.RMSPropOptimizer (TF 1.x, momentum 0, not centered) after clip_by_value(g, -clip, clip) (clip 0: none):
    ms = decay*ms + (1-decay) g^2;  p -= lr * g / sqrt(ms + eps) - eps INSIDE the root -> (p, ms), weights p / a / upd."""
    p, g, ms = _d(p), _d(g), _d(ms)
    lr, decay, eps, clip = r32(lr), r32(decay), r32(eps), r32(clip)
    if clip > 0:
        g = np.clip(g, -clip, clip)
    msn = decay * ms + (1 - decay) * g * g
    upd = lr * g / np.sqrt(msn + eps)
    return (p - upd, msn), {"p": np.abs(p) + np.abs(upd), "a": msn, "upd": np.abs(upd)}


def gauss_nll(mu, var, y, fps, scale, clip_mask=True):
    """cost.py:190-229: l = log(var_a + 1e-20) + (y - mu_a)^2 / (var_a + 1e-20) per sequence, second, frame and axis, clipped to
    [-10, 10]; loss = scale * mean_b sum l; the clip passes no gradient outside (-10, 10).  mu, var (B,3), y (B,T_y,3*fps)
    interleaved x,y,z -> (loss, dmu, dvar), (w_dmu, w_dvar), l.  clip_mask=False: the gradient WITHOUT the clip's mask."""
    mu, var, y = _d(mu), _d(var), _d(y)
    B = y.shape[0]
    ye = y.reshape(B, -1, 3)
    v = (var + r32(1e-20))[:, None, :]
    d = ye - mu[:, None, :]
    l = np.log(v) + d * d / v
    s = r32(scale)
    loss = s * np.clip(l, -10, 10).sum() / max(B, 1)
    k = ((l > -10) & (l < 10)) if clip_mask else np.ones(l.shape, bool)
    gm, gv1, gv2 = -2 * d / v * k, (1 / v) * k, d * d / (v * v) * k
    f = s / max(B, 1)
    return (loss, f * gm.sum(1), f * (gv1 - gv2).sum(1)), (f * np.abs(gm).sum(1), f * (gv1 + gv2).sum(1)), l


# (B, T_y, fps) of the Gaussian NLL cases: per = 3, one trip of the 256-element loop, a second trip with a partial wave, a third,
# more than 256 block partials, both at once; (n_pix, C) of the cross-entropy cases (70 000 rows: 274 block partials)
NLL_EDGE_SHAPES = ((1, 1, 1), (5, 1, 30), (7, 3, 30), (3, 6, 30), (257, 1, 2), (300, 3, 30))
CCE_EDGE_SHAPES = ((1, 1), (255, 30), (257, 30), (700, 64), (70000, 3))


def nll_edge_inputs(seed, B, Ty, fps):
    """Inputs of gauss_nll with all three populations present: l below -10 (var 1e-7..1e-5, |y - mu| about 1e-3), l above 10
    (outliers of +-3 on var in [0.05, 1]) and the interior; no element within 1e-3 of a clip bound (those are drawn again)
    -> (mu, var, y) fp32 and the number of elements that were drawn again."""
    rng = np.random.default_rng(seed)
    per = Ty * fps * 3
    mu = rng.uniform(-1, 1, (B, 3)).astype(np.float32)
    low = (np.arange(B * 3).reshape(B, 3) % 5) == 1
    var = np.where(low, 10.0 ** rng.uniform(-7, -5, (B, 3)), rng.uniform(0.05, 1.0, (B, 3))).astype(np.float32)
    a = np.arange(per) % 3
    m_e, v_e, low_e = mu[:, a].astype(np.float64), var[:, a].astype(np.float64), low[:, a]

    def draw():
        n = rng.standard_normal((B, per))
        d = np.where(low_e, 1e-3 * n, 0.3 * np.sqrt(v_e) * n)
        out = ~low_e & (rng.random((B, per)) < 0.17)
        return (m_e + np.where(out, np.where(rng.random((B, per)) < 0.5, 3.0, -3.0), d)).astype(np.float32)

    y = draw()
    again = 0
    for _ in range(20):
        l = gauss_nll(mu, var, y.reshape(B, Ty, 3 * fps), fps, 1.0)[2].reshape(B, per)
        bad = np.abs(np.abs(l) - 10) < 1e-3
        if not bad.any():
            break
        again += int(bad.sum())
        y = np.where(bad, draw(), y)
    return mu, var, y.reshape(B, Ty, 3 * fps), again


def nll_populations(mu, var, y, fps):
    """Shares of the elements of gauss_nll below -10, above 10 and inside, and the least distance of |l| from 10."""
    l = gauss_nll(mu, var, y, fps, 1.0)[2]
    return float((l <= -10).mean()), float((l >= 10).mean()), float(((l > -10) & (l < 10)).mean()), float(np.abs(np.abs(l) - 10).min())


def mse_dense(y, target, activation, weight=1.0, time_major=False, transpose_target=True):
    """Keras mean_squared_error behind Dense(tanh | linear): loss = w mean (y - t)^2, dpre = 2 w (y - t) / n * act'(y) ->
    (loss, dpre), w_dpre.  time_major: y (T,B,O) against a target (B,T,O) (transpose_target=False leaves it as it lies)."""
    y, t = _d(y), _d(target)
    if time_major and transpose_target:
        t = t.transpose(1, 0, 2)
    t = t.reshape(y.shape)
    n = max(y.size, 1)
    sc = r32(r32(weight) / np.float32(n))
    d = y - t
    da = 1 - y * y if activation == "tanh" else np.ones_like(y)
    wa = 1 + y * y if activation == "tanh" else np.ones_like(y)
    return ((d * d).sum() * sc, 2 * d * sc * da), 2 * np.abs(d) * sc * wa


def categorical_crossentropy(p, t, eps=1e-7):
    """Keras-2.2 categorical_crossentropy on probabilities, TensorFlow backend: q = p / sum_c p, q' = clip(q, eps, 1 - eps) with
    eps and 1 - eps rounded to fp32 (1 - 2^-23), l = -sum_c t_c log q'_c, loss = mean over rows; the clip passes no gradient
    outside (eps, 1 - eps) -> (loss, dp), w_dp, q."""
    p, t = _d(p), _d(t)
    C = p.shape[-1]
    p2, t2 = p.reshape(-1, C), t.reshape(-1, C)
    n = max(p2.shape[0], 1)
    lo, hi = r32(eps), float(np.float32(1) - np.float32(eps))
    S = p2.sum(-1, keepdims=True)
    q = p2 / S
    qc = np.clip(q, lo, hi)
    loss = -(t2 * np.log(qc)).sum() / n
    g = np.where((q > lo) & (q < hi), -t2 / qc, 0.0)
    dot = (g * q).sum(-1, keepdims=True)
    w = (np.abs(g) + np.abs(g * q).sum(-1, keepdims=True)) / S / n
    return (loss, ((g - dot) / S / n).reshape(p.shape)), w.reshape(p.shape), q.reshape(p.shape)


def cce_edge_inputs(seed, n_pix, C):
    """Rows for categorical_crossentropy: unnormalised (each scaled by uniform(0.5, 2)); every 5th row has 1e-9 under its target
    class (lower clip), every 11th is exactly one-hot (q = 1, upper clip), every 7th has a soft target -> (p, t) fp32 and the
    mask of the exactly one-hot rows."""
    rng = np.random.default_rng(seed)
    p = rng.random((n_pix, C)) + 0.01
    p /= p.sum(-1, keepdims=True)
    sc = rng.uniform(0.5, 2.0, (n_pix, 1))
    cls = rng.integers(0, C, n_pix)
    r = np.arange(n_pix)
    t = np.zeros((n_pix, C))
    t[r, cls] = 1.0
    soft = rng.random((n_pix, C)) + 0.05
    t = np.where((r % 7 == 3)[:, None], soft / soft.sum(-1, keepdims=True), t)
    tiny = r % 5 == 1
    p[r[tiny], cls[tiny]] = 1e-9
    onehot = (r % 11 == 2) | (C == 1)
    p[onehot] = 0.0
    p[r[onehot], cls[onehot]] = 1.0
    t[onehot] = 0.0
    t[r[onehot], cls[onehot]] = 1.0
    return (p * sc).astype(np.float32), t.astype(np.float32), onehot


def cce_near_clip_rows(p, onehot, eps=1e-7):
    """Rows (other than the exactly one-hot ones) with a q within 2 ulp of a clip bound: fp32 and fp64 could mask them differently."""
    q = categorical_crossentropy(p, np.zeros_like(p), eps)[2]
    lo, hi = r32(eps), float(np.float32(1) - np.float32(eps))
    near = (np.abs(q - lo) <= 2 * float(np.spacing(np.float32(lo)))) | (np.abs(q - hi) <= 2 * U24)
    return near.any(-1) & ~onehot


def xyz_sum1(p, dp0=None):
    """cost.py:20-29 under cfg.add_xyz_sum1: r = ux^2 + uy^2 + uz^2 - 1 per row of C >= 3 channels, reg = 0.5 mean r^2,
    d reg / d u_k = 2 r u_k / n added to dp0 (channels >= 3 untouched) -> (reg, dp), w_dp."""
    p = _d(p)
    C = p.shape[-1]
    p2 = p.reshape(-1, C)
    n = p2.shape[0]
    ss = (p2[:, :3] ** 2).sum(-1, keepdims=True)
    r = ss - 1
    dp = np.zeros_like(p2) if dp0 is None else _d(dp0).reshape(-1, C).copy()
    w = np.abs(dp)
    g = 2 * r * p2[:, :3] / n
    dp[:, :3] += g
    w[:, :3] += 2 * (ss + 1) * np.abs(p2[:, :3]) / n
    return (0.5 * (r * r).mean(), dp.reshape(p.shape)), w.reshape(p.shape)


def _refeed_axis(n, planar):
    fps = n // 3
    return (np.arange(n) // fps) if planar else (np.arange(n) % 3)


def sample_refeed(mu, var, noise, std="sqrt", planar=False):
    """lstm.py:460-468 / lstm_keras.py:139-149: x = mu_a + sd(var_a) * noise, sd = sqrt(var) ('sqrt') or var itself ('var');
    frames interleaved x,y,z or planar [x*fps | y*fps | z*fps] -> x (B,3*fps), w_x."""
    mu, var, noise = _d(mu), _d(var), _d(noise)
    a = _refeed_axis(noise.shape[1], planar)
    sd = np.sqrt(var) if std == "sqrt" else var
    t = sd[:, a] * noise
    return mu[:, a] + t, np.abs(mu[:, a]) + np.abs(t)


def sample_refeed_bwd(dx, var, noise, std="sqrt", planar=False, dmu0=None, dvar0=None):
    """Gradient of sample_refeed: dmu_a = sum_frames dx, dvar_a = sum_frames dx * noise * sd'(var_a), sd' = 1 / (2 sqrt(var)) or 1,
    added to dmu0 / dvar0 where given -> (dmu, dvar), (w_dmu, w_dvar)."""
    dx, var, noise = _d(dx), _d(var), _d(noise)
    a = _refeed_axis(noise.shape[1], planar)
    sel = (a[None, :] == np.arange(3)[:, None]).astype(np.float64)      # (3, n)
    sdp = 0.5 / np.sqrt(var) if std == "sqrt" else np.ones_like(var)
    gm, wm = dx @ sel.T, np.abs(dx) @ sel.T
    gv, wv = (dx * noise) @ sel.T * sdp, np.abs(dx * noise) @ sel.T * sdp
    if dmu0 is not None:
        gm, wm = gm + _d(dmu0), wm + np.abs(_d(dmu0))
    if dvar0 is not None:
        gv, wv = gv + _d(dvar0), wv + np.abs(_d(dvar0))
    return (gm, gv), (wm, wv)


# --------------------------------------------------------------------------------------
# a10: tf.contrib.rnn.LSTMCell / MultiRNNCell / tf.nn.dynamic_rnn as used by mycode/lstm.py:218-240
# (TensorFlow 1.x contrib, not in the repo; restated from its published definition: one fused
# kernel W:(F+H,4H) applied to [x, h], gate column order i, j(=g), f, o, plain sigmoid,
# forget_bias added inside the cell, state tuple (c, h)).
# --------------------------------------------------------------------------------------
def tf_lstm_cell_step(x, c, h, W, b, forget_bias=1.0):
    H = h.shape[1]
    z = np.concatenate([x, h], axis=1) @ W + b
    i, j, f, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
    c_new = sigmoid(f + forget_bias) * c + sigmoid(i) * np.tanh(j)
    h_new = sigmoid(o) * np.tanh(c_new)
    return c_new.astype(x.dtype), h_new.astype(x.dtype)


def tf_dynamic_rnn(x, cells, init_state=None, forget_bias=1.0):
    """cells: list of (W, b) per layer; init_state: (L,2,B,H) with [l,0]=c, [l,1]=h (lstm.py:128-132).
    Returns (states_series (B,T,H) of the top layer, current_state (L,2,B,H))."""
    B, T, _ = x.shape
    L = len(cells)
    H = cells[0][1].shape[0] // 4
    st = np.zeros((L, 2, B, H), x.dtype) if init_state is None else init_state.astype(x.dtype).copy()
    out = np.empty((B, T, H), x.dtype)
    for t in range(T):
        inp = x[:, t]
        for l, (W, b) in enumerate(cells):
            st[l, 0], st[l, 1] = tf_lstm_cell_step(inp, st[l, 0], st[l, 1], W, b, forget_bias)
            inp = st[l, 1]
        out[:, t] = inp
    return out, st


def tf_mean_var_head(h, head):
    """_pred_mean_var_xyz2_new (lstm.py:321-337): relu -> tanh for the means, relu -> linear -> exp for the variances."""
    mu = np.tanh(np.maximum(h @ head["mu_W1"] + head["mu_b1"], 0) @ head["mu_W2"] + head["mu_b2"])
    var = np.exp(np.maximum(h @ head["var_W1"] + head["var_b1"], 0) @ head["var_W2"] + head["var_b2"])
    return mu, var


def tf_lstm_sampled_rollout(x, cells, head, init_state, noise, forget_bias=1.0):
    """Test-time loop of lstm.py:714-740 (cfg.use_xyz, cfg.predict_mean_var): every step runs the stack over the current
    window from the state the PREVIOUS run returned, predicts (mu, var), draws one second around it
    (utility.generate_fake_batch_numpy, utility.py:73-80: normal(mu, sqrt(var)), here mu + sqrt(var) * noise[k], frames
    interleaved x,y,z by np.stack axis=-1) and shifts it into the window.  -> (mus (P,B,3), vars (P,B,3), state)."""
    win, st = x.copy(), init_state
    B, fps = x.shape[0], x.shape[2] // 3
    mus, vs = [], []
    for k in range(noise.shape[0]):
        _, st = tf_dynamic_rnn(win, cells, st, forget_bias)
        mu, var = tf_mean_var_head(st[-1, 1], head)
        mus.append(mu); vs.append(var)
        smp = (mu[:, None, :] + np.sqrt(var)[:, None, :] * noise[k].reshape(B, fps, 3)).reshape(B, 1, 3 * fps)
        win = np.concatenate([win[:, 1:], smp], axis=1)
    return np.stack(mus), np.stack(vs), st


# --------------------------------------------------------------------------------------
# a8/a9: ConvLSTM2D seq2seq (mycode/convlstm_seq2seq.py:100-282).  Keras-2.2 ConvLSTM2DCell restated:
#   x_g = conv2d(x, K_g, 'same') + b_g ;  h_g = conv2d(h, R_g, 'same')        (cross-correlation, NHWC)
#   i = s(x_i+h_i); f = s(x_f+h_f); c' = f*c + i*tanh(x_c+h_c); o = s(x_o+h_o); h' = o*tanh(c')
# kernel K:(kh,kw,C,4F), recurrent R:(kh,kw,F,4F), bias (4F), channel blocks i,f,c,o; s = hard_sigmoid
# by default (the reference never overrides it).  Dropout 0.3 on the inputs acts in training only.
# --------------------------------------------------------------------------------------
def conv2d_same(x, w, b=None, dilation=1):
    """x:(B,H,W,C), w:(kh,kw,C,N) -> (B,H,W,N); zero 'same' padding, stride 1, no kernel flip.  dilation = Keras
    `dilation_rate` (odd kernels: tap (i,j) reads the pixel (i - kh//2, j - kw//2) * dilation away)."""
    B, H, W, C = x.shape
    kh, kw, _, N = w.shape
    d = int(dilation)
    ph, pw = d * ((kh - 1) // 2), d * ((kw - 1) // 2)
    xp = np.zeros((B, H + d * (kh - 1), W + d * (kw - 1), C), x.dtype)
    xp[:, ph:ph + H, pw:pw + W] = x
    out = np.zeros((B, H, W, N), x.dtype)
    for dy in range(kh):
        for dx in range(kw):
            out += xp[:, d * dy:d * dy + H, d * dx:d * dx + W] @ w[dy, dx]
    if b is not None:
        out = out + b
    return out.astype(x.dtype)


def convlstm2d_step(x, h, c, K, R, b, act="hard_sigmoid", dilation=1):
    """Keras 2.2 ConvLSTM2DCell.call: `dilation_rate` reaches input_conv only; recurrent_conv is never dilated."""
    F = R.shape[2]
    z = conv2d_same(x, K, b, dilation) + conv2d_same(h, R)
    s = _rec_act(act)
    i, f, g, o = s(z[..., :F]), s(z[..., F:2 * F]), np.tanh(z[..., 2 * F:3 * F]), s(z[..., 3 * F:])
    c_new = f * c + i * g
    return (o * np.tanh(c_new)).astype(x.dtype), c_new.astype(x.dtype)


def convlstm2d_layer(x, K, R, b, h0=None, c0=None, act="hard_sigmoid", dilation=1):
    """x:(B,T,H,W,C) -> (hs:(B,T,H,W,F), h_T, c_T)."""
    B, T, H, W, _ = x.shape
    F = R.shape[2]
    h = np.zeros((B, H, W, F), x.dtype) if h0 is None else h0
    c = np.zeros((B, H, W, F), x.dtype) if c0 is None else c0
    hs = np.empty((B, T, H, W, F), x.dtype)
    for t in range(T):
        h, c = convlstm2d_step(x[:, t], h, c, K, R, b, act, dilation)
        hs[:, t] = h
    return hs, h, c


def softmax_last(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(x.dtype)


def convlstm_seq2seq_forward(enc_in, dec_in0, w, T_out, head="conv2d", act="hard_sigmoid", dilation=1):
    """3-layer ConvLSTM2D encoder, mirrored decoder unrolled T_out times with state hand-off, channel
    concat of the three layer outputs, head, output fed back (convlstm_seq2seq.py:100-126,146-165,209-282).
      head 'conv2d' (cfg.use_one_hot): Conv2D -> Conv2D -> Conv2D (relu each) + channel softmax
      head 'conv1d' (xyz mode, H == 1): Conv1D k=7 relu, relu, softmax over the 3 output channels
      head 'dense'  (cfg.predict_mean_var + cfg.input_mean_var, 1x1 maps of 6 channels): Flatten + Dense(6)
    dilation = cfg.dilation_rate (config.py:105), passed to the six ConvLSTM2D layers (:102,110,120,148,155,162), not to the head.
    enc_in:(B,T_in,H,W,C)  dec_in0:(B,1,H,W,C)  ->  (B,T_out,H,W,Cout)   ('dense': (B,T_out,6))."""
    x = enc_in
    states = []
    for l in range(3):
        x, h, c = convlstm2d_layer(x, w["enc%d_K" % l], w["enc%d_R" % l], w["enc%d_b" % l], act=act, dilation=dilation)
        states.append((h, c))
    inp = dec_in0[:, 0]
    outs = []
    for _ in range(T_out):
        feats = []
        cur = inp
        for l in range(3):
            h, c = convlstm2d_step(cur, states[l][0], states[l][1], w["dec%d_K" % l], w["dec%d_R" % l], w["dec%d_b" % l], act,
                                   dilation)
            states[l] = (h, c)
            feats.append(h)
            cur = h
        y = np.concatenate(feats, axis=-1)
        if head == "dense":      # cfg.predict_mean_var: Flatten + Dense(6, linear) (convlstm_seq2seq.py:171,225-227)
            y = y.reshape(y.shape[0], -1) @ w["head0_W"] + w["head0_b"]
            outs.append(y)
            # fed back as a 1x1 map of 6 channels (cfg.input_mean_var, :272-273)
            inp = y.reshape(y.shape[0], 1, 1, -1)
            continue
        y = np.maximum(conv2d_same(y, w["head0_W"], w["head0_b"]), 0)
        y = np.maximum(conv2d_same(y, w["head1_W"], w["head1_b"]), 0)
        y = conv2d_same(y, w["head2_W"], w["head2_b"])
        if head == "conv2d":
            y = softmax_last(np.maximum(y, 0))        # relu in the layer, then Softmax(axis=-1)
        else:
            y = softmax_last(y)                       # Conv1D(..., activation='softmax')
        outs.append(y)
        inp = y
    return np.stack(outs, axis=1)


def init_convlstm_seq2seq(seed, C=30, latent_dim=16, k=5, head="conv2d", head_filters=(512, 1024), dtype=np.float32,
                          map_hw=(1, 1)):
    """Keras initialisers: glorot_uniform kernels (fan = receptive field x channels), orthogonal recurrent
    kernels (flattened), unit forget bias."""
    rng = np.random.default_rng(seed)
    filters = (latent_dim * 2, latent_dim, latent_dim // 2)
    kh, kw = (k, k) if head == "conv2d" else (k, k)
    w = {}

    def glorot(shape):
        rf = int(np.prod(shape[:-2]))
        lim = np.sqrt(6.0 / (rf * shape[-2] + rf * shape[-1]))
        return rng.uniform(-lim, lim, shape).astype(dtype)

    for part in ("enc", "dec"):
        cin = C
        for l, F in enumerate(filters):
            w["%s%d_K" % (part, l)] = glorot((kh, kw, cin, 4 * F))
            w["%s%d_R" % (part, l)] = _orthogonal(rng, kh * kw * F, 4 * F, dtype).reshape(kh, kw, F, 4 * F)
            b = (0.05 * rng.standard_normal(4 * F)).astype(dtype)
            b[F:2 * F] += 1
            w["%s%d_b" % (part, l)] = b
            cin = F
    cat = sum(filters)
    if head == "dense":
        n_in = map_hw[0] * map_hw[1] * cat
        lim = np.sqrt(6.0 / (n_in + 6))
        w["head0_W"] = rng.uniform(-lim, lim, (n_in, 6)).astype(dtype)
        w["head0_b"] = (0.05 * rng.standard_normal(6)).astype(dtype)
        return w
    hk = (k, k) if head == "conv2d" else (1, 7)
    chans = (cat,) + tuple(head_filters) + ((C,) if head == "conv2d" else (3,))
    for i in range(3):
        w["head%d_W" % i] = glorot(hk + (chans[i], chans[i + 1]))
        w["head%d_b" % i] = (0.05 * rng.standard_normal(chans[i + 1])).astype(dtype)
    return w


# --------------------------------------------------------------------------------------
# the consumer of the path's output - FoV hit rate per predicted second
#   xyz2thetaphi           mycode/dataIO.py:77-82
#   boundary_cases         mycode/baseline_knn_mean.py:78-85
#   bbox_overlaps_hit_rate mycode/baseline_knn_mean.py:62-82 via get_iou_or_hitrate :48-60
# --------------------------------------------------------------------------------------
def xyz2thetaphi(x, y, z):
    theta = np.mod(np.arctan2(y, x), 2 * np.pi) - np.pi
    phi = np.mod(np.arctan2(z, np.sqrt(x ** 2 + y ** 2)) + np.pi / 2, np.pi)
    return theta, phi


def fov_hit_rate(pred_xyz, gt_xyz, span_deg=120.0, gt_span_deg=120.0):
    """pred_xyz, gt_xyz: (..., 3) FoV-centre unit vectors (per-second means).  Returns the hit rate
    = area(pred box ∩ gt box) / area(gt box) of the two (theta,phi) boxes of the given angular spans,
    with the reference's +-2pi wrap fix when the two centres straddle the theta seam."""
    pt, pp = xyz2thetaphi(pred_xyz[..., 0], pred_xyz[..., 1], pred_xyz[..., 2])
    gt, gp = xyz2thetaphi(gt_xyz[..., 0], gt_xyz[..., 1], gt_xyz[..., 2])
    pt, gt = pt.copy(), gt.copy()
    c1 = (gt > 2 / 3.0 * np.pi) & (pt < -2 / 3.0 * np.pi)
    pt[c1] += 2 * np.pi
    c2 = (gt < -2 / 3.0 * np.pi) & (pt > 2 / 3.0 * np.pi)
    gt[c2] += 2 * np.pi
    s, gs = span_deg / 180.0 * np.pi, gt_span_deg / 180.0 * np.pi
    iw = np.minimum(pt + s / 2, gt + gs / 2) - np.maximum(pt - s / 2, gt - gs / 2)
    ih = np.minimum(pp + s / 2, gp + gs / 2) - np.maximum(pp - s / 2, gp - gs / 2)
    return np.where((iw > 0) & (ih > 0), iw * ih / (gs * gs), 0.0)


# --------------------------------------------------------------------------------------
# a10, the branch mycode/config.py:8,69,71 actually selects (use_xyz, predict_mean_var = False, use_GMM = True):
# the mixture-density head _GMM_3dgassian (lstm.py:377-400) with costfunc.mixture_3d_gaussian_loss
# (cost.py:486-549, density cost.py:352-383, PSD repair cost.py:335-348), and the third branch (predict raw,
# lstm.py:147-174,486-508) with costfunc.pred_raw_loss_tf (cost.py:634-641).  TensorFlow-1.x pieces restated from
# their published definitions (tf.contrib.layers.fully_connected = x W + b then the activation;
# tf.contrib.distributions.MultivariateNormalFullCovariance.prob = the N(mu, Sigma) density; tf.self_adjoint_eig
# = ascending eigenvalues): parity unpinned like the rest of the arithmetic; the density is cross-checked
# against scipy.stats.multivariate_normal in tests/test_oracle.py.
#
# Reference quirks kept on purpose (each one changes the numbers):
#   * tf.layers.dropout(internal, rate=0.2) is called WITHOUT training=True (lstm.py:380,382): it is the
#     identity in every run of the script.  `masks` exists for a caller who wants the two dropouts.
#   * mixture_3d_gaussian_loss never multiplies by mixture_pi (cost.py:532-538: `gaussian` is the bare
#     density, the expanded mixture_pi is dropped; the 2-D loss at cost.py:466 does multiply): the 20
#     softmax weights get no gradient.  weight_by_pi=True is the textbook mixture.
#   * process_in_seconds scores only second 0 of y (cost.py:502-505) and divides by
#     batch_size * running_length * fps whatever the number of frames summed.
# --------------------------------------------------------------------------------------
GMM_KEYS = ("fc1_W", "fc1_b", "fc2_W", "fc2_b", "fc3_W", "fc3_b", "fc4_W", "fc4_b")


def tf_gmm3d_head(h, head, masks=None, n_mix=20):
    """_GMM_3dgassian: h (B,H) -> 64 relu -> 128 relu -> 256 relu -> 10*n_mix linear, split
    [n pi-logits | 3n means | 3n log-sigmas | 3n atanh-rhos].  -> (pi, us, sigmas, rhos), activations (a1,a2,a3)."""
    a1 = np.maximum(h @ head["fc1_W"] + head["fc1_b"], 0)
    if masks is not None and masks[0] is not None:
        a1 = a1 * masks[0]
    a2 = np.maximum(a1 @ head["fc2_W"] + head["fc2_b"], 0)
    if masks is not None and masks[1] is not None:
        a2 = a2 * masks[1]
    a3 = np.maximum(a2 @ head["fc3_W"] + head["fc3_b"], 0)
    pred = a3 @ head["fc4_W"] + head["fc4_b"]
    n = n_mix
    e = np.exp(pred[:, :n])                       # lstm.py:394-396: exp / sum, no max subtraction
    pi = e / e.sum(1, keepdims=True)
    return (pi, pred[:, n:4 * n], np.exp(pred[:, 4 * n:7 * n]), np.tanh(pred[:, 7 * n:10 * n])), (a1, a2, a3)


def gmm3d_covariance(sig, rho):
    """(...,3) sigmas and (...,3) rhos (rho12, rho13, rho23) -> covariance (...,3,3) after the reference's repair
    (cost.py:335-348): if the smallest eigenvalue is negative, subtract 10 * min_eig * I."""
    s1, s2, s3 = sig[..., 0], sig[..., 1], sig[..., 2]
    r12, r13, r23 = rho[..., 0], rho[..., 1], rho[..., 2]
    S = np.stack([np.stack([s1 * s1, r12 * s1 * s2, r13 * s1 * s3], -1),
                  np.stack([r12 * s1 * s2, s2 * s2, r23 * s2 * s3], -1),
                  np.stack([r13 * s1 * s3, r23 * s2 * s3, s3 * s3], -1)], -2)
    lam = np.linalg.eigvalsh(S)[..., 0]
    shift = np.where(lam < 0, -10.0 * lam, 0.0)
    return S + shift[..., None, None] * np.eye(3)


def mvn3_prob(y, mu, cov):
    """N(y; mu, cov) for y (...,3), mu (...,3), cov (...,3,3)."""
    d = y - mu
    sol = np.linalg.solve(cov, d[..., None])[..., 0]
    q = (d * sol).sum(-1)
    return np.exp(-0.5 * q) / np.sqrt((2 * np.pi) ** 3 * np.linalg.det(cov))


def mixture_3d_gaussian_loss(y_true, params, batch_size, running_length, fps=30, process_in_seconds=True,
                             weight_by_pi=False):
    """cost.py:486-549.  y_true (B,T_y,3*fps) [process_in_seconds: second 0 only] or (B,T,3) [per frame]."""
    pi, us, sig, rho = params
    B, n = pi.shape
    pts = y_true[:, 0].reshape(B, -1, 3) if process_in_seconds else y_true      # (B,P,3)
    mu = us.reshape(B, n, 3)                     # us[:, 0::3], [1::3], [2::3] = x, y, z of mixture m
    cov = gmm3d_covariance(sig.reshape(B, n, 3), rho.reshape(B, n, 3))          # (B,n,3,3)
    p = mvn3_prob(pts[:, None, :, :], mu[:, :, None, :], cov[:, :, None, :, :])  # (B,n,P)
    if weight_by_pi:
        p = p * pi[:, :, None]
    loss = -np.log(p.sum(1) + 1e-20).sum()
    return loss / batch_size / (running_length * fps if process_in_seconds else running_length)


def sample_mixture_3d(params, u, z):
    """One draw per frame from the 3-D mixture, what utility.sample_mixture_3D's docstring promises ("randomly one sample
    from 3D GMM", utility.py:178-208).  The committed function cannot run (pdb.set_trace(), a module-level batch_size
    that does not exist, 2-D indexing of 3-D parameters, a (B,1,2) result fed to a (B,1,90) placeholder), so the
    intent is restated: frame f of row b picks component m = first index with cumsum(pi)[m] > u[b,f] and draws
    mu_m + L_m z[b,f], L_m the Cholesky factor of the repaired covariance.  u (B,P) uniform, z (B,P,3) normal
    -> (B,1,3*P) interleaved x,y,z."""
    pi, us, sig, rho = params
    B, n = pi.shape
    P = u.shape[1]
    mu = us.reshape(B, n, 3)
    L = np.linalg.cholesky(gmm3d_covariance(sig.reshape(B, n, 3), rho.reshape(B, n, 3)))
    cum = np.cumsum(pi, 1)
    out = np.empty((B, P, 3), pi.dtype)
    for b in range(B):
        for f in range(P):
            m = min(int(np.searchsorted(cum[b], u[b, f], side="right")), n - 1)
            out[b, f] = mu[b, m] + L[b, m] @ z[b, f]
    return out.reshape(B, 1, 3 * P)


def tf_lstm_gmm_rollout(x, cells, head, init_state, u, z, forget_bias=1.0):
    """GMM test loop (lstm.py:690-698,735-745,820-825): only the LAST second is fed (x (B,1,90)), the state is carried,
    every step predicts the mixture and feeds back one sampled second.  u (P,B,fps), z (P,B,fps,3).
    -> (samples (P,B,1,90), final state)."""
    win, st = x.copy(), init_state
    outs = []
    for k in range(u.shape[0]):
        _, st = tf_dynamic_rnn(win, cells, st, forget_bias)
        params, _ = tf_gmm3d_head(st[-1, 1], head)
        smp = sample_mixture_3d(params, u[k], z[k])
        outs.append(smp)
        win = np.concatenate([win[:, 1:], smp], axis=1)
    return np.stack(outs), st


RAW_KEYS = ("conv1_W", "conv1_b", "conv2_W", "conv2_b", "conv3_W", "conv3_b")


def tf_raw_head(h, head):
    """pred_cnn_model_fn (lstm.py:147-174): three tf.layers.conv1d (k = 5, 'same', relu, relu, tanh; 128, 256, 3*fps
    filters) on h expanded to ONE time step.  With one step and zero padding only the centre tap k//2 of each kernel
    (k, C_in, C_out) meets data ("equivalent to 3 fc layers", :151).  -> (B,1,3*fps), activations."""
    c = head["conv1_W"].shape[0] // 2
    a1 = np.maximum(h @ head["conv1_W"][c] + head["conv1_b"], 0)
    a2 = np.maximum(a1 @ head["conv2_W"][c] + head["conv2_b"], 0)
    out = np.tanh(a2 @ head["conv3_W"][c] + head["conv3_b"])
    return out[:, None, :], (a1, a2)


def total_variation_loss_tf(pred):
    """cost.py:608-618 on (B,T,3*fps): differences along axis ONE (time steps), not along the frames of a second."""
    x, y, z = pred[:, :, 0::3], pred[:, :, 1::3], pred[:, :, 2::3]
    d = (x[:, :-1] - x[:, 1:]) ** 2 + (y[:, :-1] - y[:, 1:]) ** 2 + (z[:, :-1] - z[:, 1:]) ** 2
    return (d ** 1.25).sum()


def sum1reg_tf(pred):
    """cost.py:622-631: sum (x^2 + y^2 + z^2 - 1)^2."""
    x, y, z = pred[:, :, 0::3], pred[:, :, 1::3], pred[:, :, 2::3]
    return ((x * x + y * y + z * z - 1) ** 2).sum()


def pred_raw_loss_tf(this_y, pred, use_reg=False):
    """cost.py:634-641: tf.losses.mean_squared_error (mean over every element) + 0.1 * TV (+ 0.1 * sum-to-one).  In
    lstm.py every call passes ONE time step (:493-508), so the TV term slices an empty range and is exactly 0."""
    loss = ((this_y - pred) ** 2).mean() + 0.1 * total_variation_loss_tf(pred)
    if use_reg:
        loss = loss + 0.1 * sum1reg_tf(pred)
    return loss


def tf_lstm_raw_refeed_loss(x, y, cells, head, init_state, use_reg=False, forget_bias=1.0):
    """Training graph of the raw branch, predict_len > 1 (lstm.py:486-508): second k+1 is scored after re-running the
    stack, from the same fed state, on the window shifted by one second whose last slot is prediction k itself.
    -> (loss, predictions (P,B,1,3*fps))."""
    win, preds, loss = x, [], 0.0
    for k in range(y.shape[1]):
        _, st = tf_dynamic_rnn(win, cells, init_state, forget_bias)
        p, _ = tf_raw_head(st[-1, 1], head)
        loss = loss + pred_raw_loss_tf(y[:, k:k + 1], p, use_reg)
        preds.append(p)
        win = np.concatenate([win[:, 1:], p], axis=1)
    return loss, np.stack(preds)


# --------------------------------------------------------------------------------------
# Second half of mycode/FoV_seq2seq_no_teac_forc.py (:420-486): the unrolled no-teacher-forcing decoder whose Dense head
# also sees the OTHER users' future through a ConvLSTM2D branch.
#   encoder LSTM(latent_dim) -> (h, c) seed the decoder (:431-434; this half has no decoder_no_init_state switch)
#   ConvLSTM2D(filters = latent_dim, kernel_size = (num_user-1, 3), 'same', return_sequences) over the others' future
#       (B, T_out, num_user-1, fps, 3) from zero state (:438-448) - it does not depend on the decoder
#   step t: d_t = LSTM(x_t; h, c);  s_t = Dense(latent_dim, linear)(Flatten(convlstm output t))  (:468-470)
#           y_t = Dense(6, tanh)(concat[d_t, s_t]) (:471-472);  x_{t+1} = y_t (:476)
# --------------------------------------------------------------------------------------
OTHERS_FUTURE_ORDER = ("enc_K", "enc_R", "enc_b", "oth_K", "oth_R", "oth_b", "flat_W", "flat_b", "dec_K", "dec_R", "dec_b",
                       "dense_W", "dense_b")


def others_future_convlstm_forward(enc_in, others_fut, dec_in0, w, act="sigmoid", conv_act="hard_sigmoid"):
    """enc_in (B,T_in,F), others_fut (B,T_out,U-1,fps,3), dec_in0 (B,1,O) -> (B,T_out,O)."""
    _, h, c = lstm_layer(enc_in, w["enc_K"], w["enc_R"], w["enc_b"], act=act)
    hs, _, _ = convlstm2d_layer(others_fut, w["oth_K"], w["oth_R"], w["oth_b"], act=conv_act)     # (B,T,U-1,fps,H)
    B, T = hs.shape[:2]
    s = hs.reshape(B, T, -1) @ w["flat_W"] + w["flat_b"]          # Keras Flatten of a channels-last map: (row, column, filter)
    x, out = dec_in0[:, 0].astype(enc_in.dtype), []
    for t in range(T):
        h, c = lstm_step(x, h, c, w["dec_K"], w["dec_R"], w["dec_b"], act)
        x = np.tanh(np.concatenate([h, s[:, t]], axis=1) @ w["dense_W"] + w["dense_b"])
        out.append(x)
    return np.stack(out, axis=1)


def init_others_future_convlstm(seed, F_enc=90, F_dec=6, H=64, num_user=34, fps=30, dtype=np.float32, bias_noise=0.0):
    rng = np.random.default_rng(seed)
    w = {}
    w["enc_K"], w["enc_R"], w["enc_b"] = init_lstm(rng, F_enc, H, dtype)
    w["dec_K"], w["dec_R"], w["dec_b"] = init_lstm(rng, F_dec, H, dtype)
    kh, kw = num_user - 1, 3

    def glorot(shape):
        rf = int(np.prod(shape[:-2]))
        lim = np.sqrt(6.0 / (rf * shape[-2] + rf * shape[-1]))
        return rng.uniform(-lim, lim, shape).astype(dtype)

    w["oth_K"] = glorot((kh, kw, 3, 4 * H))
    w["oth_R"] = _orthogonal(rng, kh * kw * H, 4 * H, dtype).reshape(kh, kw, H, 4 * H)
    b = np.zeros(4 * H, dtype)
    b[H:2 * H] = 1
    w["oth_b"] = b
    n_flat = (num_user - 1) * fps * H
    w["flat_W"] = _glorot_uniform(rng, n_flat, H, dtype)
    w["flat_b"] = np.zeros(H, dtype)
    w["dense_W"] = _glorot_uniform(rng, 2 * H, F_dec, dtype)
    w["dense_b"] = np.zeros(F_dec, dtype)
    if bias_noise:
        for k in ("enc_b", "dec_b", "oth_b", "flat_b", "dense_b"):
            w[k] = (w[k] + bias_noise * rng.standard_normal(w[k].shape)).astype(dtype)
    return w


# --------------------------------------------------------------------------------------
# Value regimes (tests/test_gpu_value_regimes.py): weights, inputs and states for which stated shares of the
# pre-activations are clamped / saturated / overflowing IN THE fp64 FORWARD OF THIS FILE, and the yardstick the tests
# there measure the kernels with.  The default initialisers above keep a gate pre-activation near a standard deviation
# of 0.3: no element ever meets the clamp of hard_sigmoid, a saturated sigmoid / tanh or a large cell state.
# The spread sits on the BIAS (a wide normal) and on x K; the recurrent kernel stays orthogonal at gain `r_gain` (1-2, one
# bf16 case at 4): a large recurrent gain that is not fully saturated makes the recurrence chaotic, fp32 and fp64 then part
# ways for legitimate reasons and no bound means anything.  With the saturation coming from x K + b the step stays
# contractive.
#   R1 clamped      hard_sigmoid: about half of the i / f / o pre-activations beyond +-2.5, the rest on the linear piece
#   R2 saturated    sigmoid: >= 20 % of the gate pre-activations beyond +-17 (fp32 sigmoid is 0 / 1), >= 20 % of the
#                   arguments of tanh beyond +-9 (fp32 tanh is +-1): g through the bias; c through a wide initial cell state on
#                   the 35 % of the units whose forget bias pins f at 1 ("trained forget gates sit at 1").  The other units start
#                   from a cell state of order 1: an error dz in a forget gate ON ITS SLOPE reaches c as |c_prev| s'(z) dz, so a
#                   wide c_prev there would turn the last bit of a 256-term sum (1e-6, and dependent on its order) into an error
#                   of the size of the written 2e-5 - a statement about summation order, not about the kernel
#   R3 overflow     R2 plus rows `extreme` of the first 16-sequence tile whose pre-activations pass +-100 and +-200 (exp
#                   overflows to inf on one side and flushes to 0 on the other): the last input feature is theirs alone (zero in
#                   every other row), its kernel row is +-1, and they carry +-A on it (A = 130 / 300, sign alternating in time;
#                   one row ordinary until mid-sequence).  EVERY pre-activation of such a row moves by A, so that none of its
#                   elements is a cancellation of partial sums of magnitude 32 .. 64 that lands back on a slope: such an element
#                   carries half an ulp of the partial sum per accumulation step, in an order-dependent way (1.5e-5 over 64 steps),
#                   against a written bound of 2e-5.  `x_edge` is a second batch for the SAME K, R with a zero bias `b_edge`: its
#                   second tile is all zero (inputs and state), its last tile holds inputs of order 1e-6 from zero state (tanh
#                   cancels: absolute bounds only)
#   R4 accumulating forget gate pinned at 1, i * g of one sign per unit through the bias, zero initial state: |c| grows
#                   linearly with T (T = 256: max |c| passes 50)
# --------------------------------------------------------------------------------------
REGIMES = ("R1", "R2", "R3", "R4")
REGIME_ACT = {"R1": "hard_sigmoid", "R2": "sigmoid", "R3": "sigmoid", "R4": "sigmoid"}
_REGIME_SPREAD = {      # bias std of (i, f, g, o), std of x K, share of units with the forget gate pinned at 1
    "R1": ((3.0, 3.0, 3.0, 3.0), 1.5, 0.0),
    "R2": ((20.0, 20.0, 20.0, 20.0), 4.0, 0.35),
    "R3": ((20.0, 20.0, 20.0, 20.0), 4.0, 0.35),
}
FORGET_PINNED = 30.0    # a forget bias from here on: f = 1.0 exactly in fp32 whatever x K + h R add (|.| < 12)


def regime_layer(rng, F, H, regime, x_rms, r_gain=1.0, act=None, dtype=np.float32, xk=None):
    """K (F,4H), R (H,4H), b (4H,) of one layer in `regime`, for inputs whose elements have root mean square `x_rms`.
    xk: the spread of x K, overriding the regime's.  A layer whose input is COMPUTED (a hidden state, a fed-back output) keeps it
    at 0.25 .. 0.5: in the bf16 kernels such an input is rounded to 8 bits before the product, an element on a rounding boundary
    may round either way, and one bf16 ulp times a large K would move a pre-activation by more than the bound it is held to."""
    R = (r_gain * _orthogonal(rng, H, 4 * H, np.float64)).astype(dtype)
    b = np.empty(4 * H)
    if regime == "R4":
        hard = act_code(act or REGIME_ACT[regime]) == ACT_HARD_SIGMOID
        sgn = np.where(rng.random(H) < 0.5, -1.0, 1.0)
        b[:H] = rng.normal(2.0, 0.5, H)                       # i in (0.6, 1)
        b[H:2 * H] = 10.0 if hard else 30.0                   # f = 1.0 exactly in both formats
        b[2 * H:3 * H] = sgn * rng.uniform(1.5, 2.5, H)       # g of one sign per unit (h R stays below 1.5)
        b[3 * H:] = rng.normal(0.0, 1.0, H)
        xk = 0.15                                             # (its own, below the ordinary spread: the sign of g must hold)
    else:
        sb, xk0, pinned = _REGIME_SPREAD[regime]
        xk = xk0 if xk is None else xk
        for q in range(4):
            b[q * H:(q + 1) * H] = rng.normal(0.0, sb[q], H)
        bf = b[H:2 * H]
        bf[bf >= FORGET_PINNED - 15.0] -= 15.0                 # nothing in between: a unit is pinned or well below the pin
        pin = rng.permutation(H) < int(np.ceil(pinned * H))
        bf[pin] = rng.uniform(FORGET_PINNED, FORGET_PINNED + 15.0, int(pin.sum()))
    K = rng.normal(0.0, xk / (np.sqrt(F) * x_rms), (F, 4 * H))
    return K.astype(dtype), R, b.astype(dtype)


def regime_state(rng, B, b, regime, dtype=np.float32):
    """(h0, c0) (B,H) for a layer with bias b: h0 inside (-1, 1); c0 of order 1, and +-(12 .. 40) on the units whose forget gate
    is pinned at 1 (R2 / R3)."""
    H = b.shape[0] // 4
    h0 = np.clip(0.5 * rng.standard_normal((B, H)), -1, 1)
    c0 = 0.5 * rng.standard_normal((B, H))
    pin = b[H:2 * H] >= FORGET_PINNED
    if regime in ("R2", "R3") and pin.any():
        wide = rng.uniform(12.0, 40.0, (B, H)) * np.where(rng.random((B, H)) < 0.5, -1.0, 1.0)
        c0 = np.where(pin[None, :], wide, c0)
    return h0.astype(dtype), c0.astype(dtype)


BF16_XK = 0.3    # the spread of x K in the bf16 cases: the ordinary one (Glorot K, inputs in (-1, 1)).  The product's operands round to 8
# bits, the bias is added in fp32 and never rounded: with the whole spread on the bias the bf16 kernels stay within the 5e-3 of the
# FULL-precision oracle that tests/test_gpu_bf16.py holds them to, and the value-regime cases assert it too


def regime_lstm(seed, F, H, regime, B, T, act=None, r_gain=1.0, state=True, dtype=np.float32, xk=None):
    """One LSTM layer's case in a value regime -> dict(K, R, b, x (B,T,F), h0, c0 (B,H) or None, act, regime) and, for R3,
    extreme (row indices), x_edge, b_edge.  state=False: zero initial state (entry points that take none); R2 / R3 then
    saturate tanh through g alone."""
    assert regime in REGIMES
    act = act or REGIME_ACT[regime]
    rng = np.random.default_rng(seed)
    K, R, b = regime_layer(rng, F, H, regime, 1.0 / np.sqrt(3.0), r_gain, act, dtype, xk=xk)
    x = rng.uniform(-1, 1, (B, T, F)).astype(dtype)
    p = {"K": K, "R": R, "b": b, "x": x, "h0": None, "c0": None, "act": act, "regime": regime}
    if regime != "R4" and state:
        p["h0"], p["c0"] = regime_state(rng, B, b, regime, dtype)
    if regime == "R3":
        assert B > 16
        rows = np.array([3, 9, 12])
        p["extreme"] = rows
        K[F - 1] = np.where(rng.random(4 * H) < 0.5, -1.0, 1.0)      # the extreme rows' own feature
        x[:, :, F - 1] = 0
        for r, A, t0 in ((rows[0], 130.0, 0), (rows[1], 300.0, 0), (rows[2], 300.0, T // 2)):   # ordinary until t0, then extreme
            x[r, t0:, F - 1] = A * (-1.0) ** np.arange(t0, T)
        xe = x.copy()
        xe[:, :, F - 1] = 0
        xe[16:32] = 0
        xe[32:] = rng.uniform(-1e-6, 1e-6, xe[32:].shape)
        p["x_edge"], p["b_edge"] = xe.astype(dtype), np.zeros_like(b)
    return p


def regime_preactivations(x, K, R, b, hs, h0=None, bf16=False):
    """z (B,T,4H) of a forward whose hidden states are hs: x_t K + b + h_{t-1} R (bf16: operands rounded as the bf16 kernels do)."""
    B, T, _ = x.shape
    H = R.shape[0]
    hp = np.concatenate([(np.zeros((B, 1, H), x.dtype) if h0 is None else h0[:, None]), hs[:, :-1]], axis=1)
    r = _rb_if(bf16)
    return r(x) @ r(K) + b + r(hp) @ r(R)


def regime_shares(p, rows=None):
    """Shares of the fp64 forward of case p (rows: a subset of the batch): gate_clamped (i / f / o beyond +-2.5),
    gate_sat (beyond +-17), g_sat / c_sat / tanh_sat (arguments of tanh beyond +-9: g's, c's, both pooled), z100 / z200
    (any pre-activation beyond +-100 / +-200, and the smaller of the two signs' shares), c_max."""
    f = lambda a: None if a is None else np.asarray(a, np.float64)
    x, K, R, b, h0, c0 = (f(p[k]) for k in ("x", "K", "R", "b", "h0", "c0"))
    hs, _, _, res = lstm_layer_train(x, K, R, b, h0, c0, act=p["act"])
    z = regime_preactivations(x, K, R, b, hs, h0)
    if rows is not None:
        z, res = z[rows], res[rows]
    H = R.shape[0]
    gates = np.concatenate([z[..., :2 * H], z[..., 3 * H:]], axis=-1)
    zg, c = z[..., 2 * H:3 * H], res[:, :, 4]
    two = lambda t: float(min((z > t).mean(), (z < -t).mean()))
    return {"gate_clamped": float((np.abs(gates) > 2.5).mean()), "gate_sat": float((np.abs(gates) > 17).mean()),
            "g_sat": float((np.abs(zg) > 9).mean()), "c_sat": float((np.abs(c) > 9).mean()),
            "tanh_sat": float((np.abs(np.concatenate([zg, c], axis=-1)) > 9).mean()),
            "z100": two(100.0), "z200": two(200.0), "c_max": float(np.abs(c).max())}


# The yardstick.  Written bounds, as a weight per element (error / weight <= 1 is the bound):
#   "f32"   fp32 values: 1e-3 |ref| + 1e-5 per element AND 2e-5 absolute, per unit of magnitude for a cell state that leaves
#           (-1, 1): 2e-5 max(1, |ref|)                                  (assert_parity of tests/test_gpu_parity.py)
#   "abs"   2e-5 absolute alone (inputs of order 1e-6: tanh cancels)
#   "bf16"  1e-3 max(1, |ref|) against the bf16-operand restatement      (TIGHT of tests/test_gpu_bf16.py)
#   a float gradients: that fraction of the tensor's max |ref| (+ 1e-9)  (1e-4 fp32; 1e-3 / 2e-3 bf16)
def regime_error(got, ref, kind):
    """max over the elements of |got - ref| / (written bound): <= 1 means the written bound holds."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    a = np.abs(ref)
    if kind == "f32":
        w = np.minimum(1e-3 * a + 1e-5, 2e-5 * np.maximum(1.0, a))
    elif kind == "abs":
        w = 2e-5
    elif kind == "bf16":
        w = 1e-3 * np.maximum(1.0, a)
    else:
        w = float(kind) * (a.max() if a.size else 0.0) + 1e-9
    return float((np.abs(got - ref) / w).max()) if got.size else 0.0


REGIME_YARDSTICK = 8.0      # fov_common.h documents 3e-7 absolute for tanh_f / sigmoid_f, NumPy's half ulp at 1 is 6e-8: a
REGIME_YARDSTICK_CAP = 10.0  # factor of 5, rounded up to a power of two.  8 e_ref may not pass 10 written bounds.


def regime_bound(e_ref):
    """The asserted bound in units of the written one: max(1, 8 e_ref)."""
    return max(1.0, REGIME_YARDSTICK * e_ref)


def _cast(p, dt):
    return [None if p[k] is None else np.asarray(p[k], dt) for k in ("x", "K", "R", "b", "h0", "c0")]


def regime_forward_tensors(hs, hT, cT, res):
    out = {"hs": hs, "hT": hT, "cT": cT}
    if res is not None:
        out.update({n: res[:, :, q] for q, n in enumerate("ifgoc")})
    return out


def regime_forward_reference(p, bf16=False, x=None, b=None):
    """-> (ref, e_ref): the fp64 forward tensors (hs, hT, cT, i, f, g, o, c) of case p and, per tensor, the disagreement of
    the SAME functions run on fp32 arrays, in units of the written bound.  bf16: both runs round the operands of the two
    products (lstm_layer_train(round_fwd=True))."""
    q = dict(p)
    if x is not None:
        q["x"], q["b"], q["h0"], q["c0"] = x, b, None, None
    kind = "bf16" if bf16 else ("abs" if x is not None else "f32")
    a64, a32 = _cast(q, np.float64), _cast(q, np.float32)
    r64 = regime_forward_tensors(*lstm_layer_train(*a64, act=p["act"], round_fwd=bf16))
    r32 = regime_forward_tensors(*lstm_layer_train(*a32, act=p["act"], round_fwd=bf16))
    return r64, {k: regime_error(r32[k], r64[k], kind) for k in r64}


GRAD_KEYS = ("dz", "dx", "dK", "dR", "db", "dh0", "dc0")


def regime_upstream(seed, B, T, H, dtype=np.float32):
    rng = np.random.default_rng(seed)
    return tuple((0.1 * rng.standard_normal(s)).astype(dtype) for s in ((B, T, H), (B, H), (B, H)))


def regime_grad_bounds(bf16):
    return {k: ((2e-3 if k == "dh0" else 1e-3) if bf16 else 1e-4) for k in GRAD_KEYS}


def regime_backward_reference(p, hs, res, ups, bf16=False, dt=np.float64):
    """lstm_layer_backward of case p on the tape (hs, res) cast to dt; bf16: the products the bf16 BPTT kernel rounds."""
    x, K, R, _, h0, c0 = _cast(p, dt)
    c = lambda a: np.asarray(a, dt)
    return lstm_layer_backward(x, K, R, h0, c0, c(hs), c(res), c(ups[0]), c(ups[1]), c(ups[2]), act=p["act"],
                               round_rec=bf16, round_dx=bf16, round_wgrad=bf16)


def regime_backward_e_ref(p, ups, bf16=False):
    """Per gradient, the disagreement (in written bounds) of lstm_layer_backward in fp64 and on fp32 arrays, both fed the
    tape of the fp32 forward of this file: one tape, so both sides take the same branch of every derivative."""
    hs, _, _, res = lstm_layer_train(*_cast(p, np.float32), act=p["act"], round_fwd=bf16)
    g64 = regime_backward_reference(p, hs, res, ups, bf16, np.float64)
    g32 = regime_backward_reference(p, hs, res, ups, bf16, np.float32)
    tol = regime_grad_bounds(bf16)
    return {k: regime_error(g32[k], g64[k], tol[k]) for k in GRAD_KEYS}


# ---- models built from regime layers --------------------------------------------------------------------------------
DENSE_SATURATING_BIAS = (12.0, -12.0, 3.0, -3.0, 0.5, -0.5)   # a tanh head whose outputs sit at +-1, near it, and on the slope


def _regime_head(rng, H, O, dtype):
    """Dense(O, tanh) head at gain 1 whose spread sits on the bias: the fed-back output saturates without a loop gain above 1."""
    W = rng.normal(0.0, 1.0 / np.sqrt(H), (H, O)).astype(dtype)
    return W, np.resize(np.array(DENSE_SATURATING_BIAS), O).astype(dtype)


def regime_seq2seq(seed, regime, B, T_in, H=256, F_enc=90, F_dec=6, r_gain=1.0, dtype=np.float32, xk=None):
    """Target-only seq2seq (init_seq2seq's keys) with the encoder and the DECODER in `regime` (R1 / R2) and a saturating head.
    -> (w, enc_in (B,T_in,F_enc), dec_in0 (B,1,F_dec), act)."""
    assert regime in ("R1", "R2")
    rng = np.random.default_rng(seed)
    w = {}
    w["enc_K"], w["enc_R"], w["enc_b"] = regime_layer(rng, F_enc, H, regime, 1.0 / np.sqrt(3.0), r_gain, None, dtype, xk=xk)
    w["dec_K"], w["dec_R"], w["dec_b"] = regime_layer(rng, F_dec, H, regime, 0.8, r_gain, None, dtype, xk=0.25)
    w["dense_W"], w["dense_b"] = _regime_head(rng, H, F_dec, dtype)
    enc = rng.uniform(-1, 1, (B, T_in, F_enc)).astype(dtype)
    dec0 = rng.uniform(-1, 1, (B, 1, F_dec)).astype(dtype)
    return w, enc, dec0, REGIME_ACT[regime]


def regime_decode(enc, dec0, w, T_out, act, bf16=False, dt=np.float64):
    """seq2seq_decode in dtype dt, also returning the decoder's pre-activations: -> dict(out (B,T_out,O), hT, cT, z (B,T_out,4H),
    pre (B,T_out,O) = the head's arguments of tanh, c (B,T_out,H)).  bf16: every product with x or h on its left rounds both
    operands (the fused bf16 call)."""
    c_ = lambda a: np.asarray(a, dt)
    w = {k: c_(v) for k, v in w.items()}
    rnd = round_bf16 if bf16 else (lambda a: a)
    if bf16:
        with bf16_operands():
            _, h, c = lstm_layer(c_(enc), w["enc_K"], w["enc_R"], w["enc_b"], act=act)
    else:
        _, h, c = lstm_layer(c_(enc), w["enc_K"], w["enc_R"], w["enc_b"], act=act)
    y = c_(dec0)[:, 0]
    H = h.shape[1]
    s = _rec_act(act)
    out, zs, pres, cs = [], [], [], []
    for _ in range(T_out):
        z = rnd(y) @ rnd(w["dec_K"]) + w["dec_b"] + rnd(h) @ rnd(w["dec_R"])
        c = s(z[:, H:2 * H]) * c + s(z[:, :H]) * np.tanh(z[:, 2 * H:3 * H])
        h = s(z[:, 3 * H:]) * np.tanh(c)
        pre = rnd(h) @ rnd(w["dense_W"]) + w["dense_b"]
        y = np.tanh(pre)
        out.append(y); zs.append(z); pres.append(pre); cs.append(c)
    st = lambda v: np.stack(v, axis=1)
    return {"out": st(out), "hT": h, "cT": c, "z": st(zs), "pre": st(pres), "c": st(cs)}


def regime_stack2(seed, regime, B, T, F=90, H=512, state=True, dtype=np.float32, xk=None):
    """Two stacked layers, both in `regime`: -> (layers [(K, R, b)] * 2, x (B,T,F), states [(h0, c0) or None] * 2, act, p1) with
    p1 the first layer's regime_lstm case (R3: its extreme rows and edge batch)."""
    p1 = regime_lstm(seed, F, H, regime, B, T, state=state, dtype=dtype, xk=xk)
    rng = np.random.default_rng(seed + 1000)
    l2 = regime_layer(rng, H, H, regime, 0.5, 1.0, None, dtype, xk=0.5)
    st = [None, None]
    if p1["h0"] is not None:
        st[0] = (p1["h0"], p1["c0"])
        st[1] = regime_state(rng, B, l2[2], regime, dtype)
    return [(p1["K"], p1["R"], p1["b"]), l2], p1["x"], st, p1["act"], p1


def regime_mix_decoder(seed, regime, B, T, H=256, O=6, dtype=np.float32):
    """The fused others-mixing decoder's inputs with both layers in `regime`: -> (w, mix_Wp (O,O), states [h1, c1, h2, c2],
    dec0 (B,O), oth_proj (B,T,O), act, extra).  R3 reaches LAYER 1 AND THE HEAD only: row 9's first input is +-500 (layer 1's
    pre-activations of step 0 pass +-100 and +-200), row 3's others-projection is scaled by 100 (the mixing tanh's arguments pass
    +-200 at every step); layer 2 reads a hidden state in (-1, 1) and every later input is a tanh output.  extra (R3): rows (3, 9),
    dec0_calm / oth_calm (the two rows ordinary), and an edge batch under zero biases (w_edge) whose second tile is all zero:
    dec0_edge, oth_edge, st_edge."""
    rng = np.random.default_rng(seed)
    w = {}
    w["dec1_K"], w["dec1_R"], w["dec1_b"] = regime_layer(rng, O, H, regime, 0.8, 1.0, None, dtype, xk=0.25)
    w["dec2_K"], w["dec2_R"], w["dec2_b"] = regime_layer(rng, H, H, regime, 0.5, 1.0, None, dtype, xk=0.5)
    w["dense_W"], w["dense_b"] = _regime_head(rng, H, O, dtype)
    mix_Wp = (0.5 * rng.standard_normal((O, O))).astype(dtype)
    st = list(regime_state(rng, B, w["dec1_b"], regime, dtype) + regime_state(rng, B, w["dec2_b"], regime, dtype))
    dec0 = rng.uniform(-1, 1, (B, O)).astype(dtype)
    oth = (np.resize(np.array(DENSE_SATURATING_BIAS), O) / 2 + 0.3 * rng.standard_normal((B, T, O))).astype(dtype)
    extra = {}
    if regime == "R3":
        assert B > 16
        extra = {"rows": np.array([3, 9]), "dec0_calm": dec0.copy(), "oth_calm": oth.copy()}
        oth[3] *= 100.0
        dec0[9] = np.where(dec0[9] < 0, -500.0, 500.0)
        de, oe, se = extra["dec0_calm"].copy(), extra["oth_calm"].copy(), [a.copy() for a in st]
        for a in [de, oe] + se:
            a[16:32] = 0
        extra.update(dec0_edge=de, oth_edge=oe, st_edge=se,
                     w_edge={k: (np.zeros_like(v) if k.endswith("_b") else v) for k, v in w.items()})
    return w, mix_Wp, st, dec0, oth, REGIME_ACT[regime], extra


def mix_decoder_preactivations(tape, dec0, st, oth_proj, w, mix_Wp, bf16=False):
    """The pre-activations of a decoder forward whose tapes are `tape` (mix_decoder_train_forward's, any float dtype):
    -> z1, z2 (T,B,4H) of the two layers and pre_m (T,B,O), the mixing tanh's arguments.  bf16: the operands the bf16 kernel
    rounds."""
    r = _rb_if(bf16)
    B = dec0.shape[0]
    x = np.concatenate([dec0.reshape(1, B, -1), tape["M"][:-1]])
    h1p = np.concatenate([st[0][None], tape["H1"][:-1]])
    h2p = np.concatenate([st[2][None], tape["H2"][:-1]])
    z1 = r(x) @ r(w["dec1_K"]) + w["dec1_b"] + r(h1p) @ r(w["dec1_R"])
    z2 = r(tape["H1"]) @ r(w["dec2_K"]) + w["dec2_b"] + r(h2p) @ r(w["dec2_R"])
    return z1, z2, tape["P"] @ mix_Wp + np.swapaxes(oth_proj, 0, 1)


def regime_tape_shares(res, act):
    """The shares of regime_shares read off a tape of ACTIVATED values res (..., 5, H) = i, f, g, o, c (fp64): a hard_sigmoid
    gate is exactly 0 / 1 iff its pre-activation lies beyond +-2.5; sigmoid(17) = 1 - 4.14e-8 and tanh(9) = 1 - 3.05e-8."""
    gates = np.stack([res[..., 0, :], res[..., 1, :], res[..., 3, :]])
    g, c = res[..., 2, :], res[..., 4, :]
    if act_code(act) == ACT_HARD_SIGMOID:
        clamped = float(((gates == 0) | (gates == 1)).mean())
        sat = 0.0
    else:
        s17 = float(sigmoid(np.array([17.0]))[0])
        sat = float(((gates > s17) | (gates < 1 - s17)).mean())
        clamped = float(((gates > float(sigmoid(np.array([2.5]))[0])) | (gates < float(sigmoid(np.array([-2.5]))[0]))).mean())
    g_sat, c_sat = float((np.abs(g) > np.tanh(9.0)).mean()), float((np.abs(c) > 9).mean())
    return {"gate_clamped": clamped, "gate_sat": sat, "g_sat": g_sat, "c_sat": c_sat, "tanh_sat": 0.5 * (g_sat + c_sat),
            "c_max": float(np.abs(c).max())}


def regime_stack2_forward(layers, x, states, act, dt=np.float64, bf16=False):
    """-> [(hs, hT, cT, res)] * 2 of two stacked layers in dtype dt (layer 2 reads layer 1's hs)."""
    c_ = lambda a: None if a is None else np.asarray(a, dt)
    out, inp = [], c_(x)
    for (K, R, b), st in zip(layers, states):
        h0, c0 = (None, None) if st is None else st
        out.append(lstm_layer_train(inp, c_(K), c_(R), c_(b), c_(h0), c_(c0), act=act, round_fwd=bf16))
        inp = out[-1][0]
    return out


def regime_stack2_upstream(seed, B, T, H, dtype=np.float32):
    """dhs2 (B,T,H), dhT2, dcT2, dhT1, dcT1 (B,H)."""
    rng = np.random.default_rng(seed)
    return tuple((0.1 * rng.standard_normal(s)).astype(dtype) for s in ((B, T, H),) + ((B, H),) * 4)


def regime_stack2_backward(layers, x, states, tapes, ups, act, dt=np.float64):
    """BPTT of the two stacked layers on the tapes [(hs1, res1), (hs2, res2)] cast to dt: layer 2 from (dhs2, dhT2, dcT2), its
    dx is layer 1's dhs.  -> dict(dz1, dz2, dK1, dR1, db1, dK2, dR2, db2, dh0_1, dc0_1, dh0_2, dc0_2)."""
    c_ = lambda a: None if a is None else np.asarray(a, dt)
    (K1, R1, _), (K2, R2, _) = layers
    s1, s2 = ((None, None) if s is None else s for s in states)
    (hs1, res1), (hs2, res2) = tapes
    dhs2, dhT2, dcT2, dhT1, dcT1 = (c_(u) for u in ups)
    g2 = lstm_layer_backward(c_(hs1), c_(K2), c_(R2), c_(s2[0]), c_(s2[1]), c_(hs2), c_(res2), dhs2, dhT2, dcT2, act=act)
    g1 = lstm_layer_backward(c_(x), c_(K1), c_(R1), c_(s1[0]), c_(s1[1]), c_(hs1), c_(res1), g2["dx"], dhT1, dcT1, act=act)
    out = {}
    for n, g in (("1", g1), ("2", g2)):
        out.update({"dz" + n: g["dz"], "dK" + n: g["dK"], "dR" + n: g["dR"], "db" + n: g["db"], "dh0_" + n: g["dh0"],
                    "dc0_" + n: g["dc0"]})
    return out


def keras_to_tf_cell(K, R, b, forget_bias=1.0):
    """(K, R, b) in Keras' gate order i, f, c, o -> tf.contrib LSTMCell's (W (F+H,4H), b) in its order i, j, f, o; the cell adds
    forget_bias itself."""
    H = R.shape[0]
    W = np.concatenate([K, R], axis=0)
    blk = lambda a, q: a[..., q * H:(q + 1) * H]
    Wt = np.concatenate([blk(W, 0), blk(W, 2), blk(W, 1), blk(W, 3)], axis=-1)
    bt = np.concatenate([blk(b, 0), blk(b, 2), blk(b, 1) - b.dtype.type(forget_bias), blk(b, 3)])
    return Wt, bt


def regime_convlstm_cell(seed, B, H, W, C, F, k, act, dtype=np.float32):
    """One ConvLSTM2D step in R3: a wide bias (saturated gates), a wide cell state on the channels whose forget gate is pinned at
    1, and in map 0 three pixels, far apart, that carry +-A (130, 300, 300) on the last input channel - theirs alone, with kernel
    taps of +-1 - so that every pre-activation under their taps passes +-100 / +-200 (see R3 above).
    -> dict(K, R, b, x, h, c, act, x_calm (the extreme pixels removed), b_edge (zeros), x_edge / h_edge / c_edge (last batch
    element all zero))."""
    rng = np.random.default_rng(seed)
    hard = act_code(act) == ACT_HARD_SIGMOID
    K = (rng.standard_normal((k, k, C, 4 * F)) / np.sqrt(k * k * C)).astype(dtype)
    K[:, :, C - 1] = np.where(rng.random((k, k, 4 * F)) < 0.5, -1.0, 1.0)
    R = (rng.standard_normal((k, k, F, 4 * F)) / np.sqrt(k * k * F)).astype(dtype)
    b = rng.normal(0.0, 3.0 if hard else 20.0, 4 * F)
    pin = rng.permutation(F) < int(np.ceil(0.35 * F))
    b[F:2 * F][pin] = 10.0 if hard else FORGET_PINNED
    b = b.astype(dtype)
    x = rng.standard_normal((B, H, W, C)).astype(dtype)
    x[..., C - 1] = 0
    h = np.clip(0.5 * rng.standard_normal((B, H, W, F)), -1, 1).astype(dtype)
    wide = rng.uniform(12.0, 40.0, (B, H, W, F)) * np.where(rng.random((B, H, W, F)) < 0.5, -1.0, 1.0)
    c = np.where(pin, wide, 0.5 * rng.standard_normal((B, H, W, F))).astype(dtype)
    x_calm = x.copy()
    for n, (y, xx) in enumerate(((H // 2, W // 2), (0, 0), (H - 1, W - 1))):
        x[0, y, xx, C - 1] = (300.0 if n else 130.0) * (-1.0) ** n
    xe, he, ce = x_calm.copy(), h.copy(), c.copy()
    xe[-1], he[-1], ce[-1] = 0, 0, 0
    return {"K": K, "R": R, "b": b, "x": x, "h": h, "c": c, "act": act, "x_calm": x_calm, "b_edge": np.zeros_like(b),
            "x_edge": xe, "h_edge": he, "c_edge": ce}


def regime_convlstm_reference(p, dt=np.float64, x=None, b=None, h=None, c=None):
    """-> dict(h, c, gates (B,H,W,4F) activated i, f, g, o, z (pre-activations)) of one ConvLSTM2D step in dtype dt."""
    c_ = lambda a: np.asarray(a, dt)
    x, b = c_(p["x"] if x is None else x), c_(p["b"] if b is None else b)
    h, c = c_(p["h"] if h is None else h), c_(p["c"] if c is None else c)
    F = p["R"].shape[2]
    z = conv2d_same(x, c_(p["K"]), b) + conv2d_same(h, c_(p["R"]))
    s = _rec_act(p["act"])
    gates = np.concatenate([s(z[..., :F]), s(z[..., F:2 * F]), np.tanh(z[..., 2 * F:3 * F]), s(z[..., 3 * F:])], axis=-1).astype(dt)
    cn = gates[..., F:2 * F] * c + gates[..., :F] * gates[..., 2 * F:3 * F]
    return {"h": (gates[..., 3 * F:] * np.tanh(cn)).astype(dt), "c": cn.astype(dt), "gates": gates, "z": z}


# --------------------------------------------------------------------------------------
# The one-tile decoders (tests/test_tile_decoders_host.py, tests/test_gpu_tile_decoders.py): the 2- and 3-layer decode
# (fov_stacked_seq2seq_decode_fwd) and the self-fed decoder with its BPTT (fov_selffed_decoder_fwd / _bwd) in the value regimes
# above, references that keep every pre-activation, and a BPTT written out on GIVEN tapes.  The references take `mistake`: a
# named way of being wrong on purpose (finite, plausible), with which the host tests show what the GPU checks can see.
# --------------------------------------------------------------------------------------
def regime_stacked_seq2seq(seed, regime, L, H, F_enc, F_dec, B, T_in, dtype=np.float32):
    """L-layer target-only seq2seq (stacked_seq2seq_forward's keys) with every layer of both sides in `regime` (R1 / R2 / R3) and
    a saturating head.  Layer 0 of each side as regime_seq2seq builds its layers; the layers above read a computed hidden state
    (regime_layer(rng, H, H, regime, 0.5, xk=0.5)).  -> dict(w, enc (B,T_in,F_enc), dec0 (B,1,F_dec), act, regime) and, for R3,
    regime_lstm's extreme rows on the encoder's last input feature: extreme, enc_calm (that feature zero in every row), and an edge
    batch for the same weights under zero LSTM biases (w_edge): enc_edge / dec0_edge, whose second tile is all zero and whose rows
    from 32 on hold inputs of order 1e-6."""
    assert regime in ("R1", "R2", "R3")
    rng = np.random.default_rng(seed)
    w = {}
    for side, F0, rms, xk in (("enc", F_enc, 1.0 / np.sqrt(3.0), None), ("dec", F_dec, 0.8, 0.25)):
        for l in range(L):
            lay = regime_layer(rng, F0, H, regime, rms, 1.0, None, dtype, xk=xk) if l == 0 else \
                regime_layer(rng, H, H, regime, 0.5, 1.0, None, dtype, xk=0.5)
            w["%s%d_K" % (side, l)], w["%s%d_R" % (side, l)], w["%s%d_b" % (side, l)] = lay
    w["dense_W"], w["dense_b"] = _regime_head(rng, H, F_dec, dtype)
    enc = rng.uniform(-1, 1, (B, T_in, F_enc)).astype(dtype)
    dec0 = rng.uniform(-1, 1, (B, 1, F_dec)).astype(dtype)
    p = {"w": w, "enc": enc, "dec0": dec0, "act": REGIME_ACT[regime], "regime": regime}
    if regime == "R3":
        assert B > 32 and F_enc >= 2 and T_in >= 2
        rows = np.array([3, 9, 12])
        p["extreme"] = rows
        w["enc0_K"][F_enc - 1] = np.where(rng.random(4 * H) < 0.5, -1.0, 1.0)
        enc[:, :, F_enc - 1] = 0
        p["enc_calm"] = enc.copy()
        for r, A, t0 in ((rows[0], 130.0, 0), (rows[1], 300.0, 0), (rows[2], 300.0, T_in // 2)):
            enc[r, t0:, F_enc - 1] = A * (-1.0) ** np.arange(t0, T_in)
        ee, de = p["enc_calm"].copy(), dec0.copy()
        ee[16:32], de[16:32] = 0, 0
        ee[32:] = rng.uniform(-1e-6, 1e-6, ee[32:].shape)
        p["enc_edge"], p["dec0_edge"] = ee.astype(dtype), de
        p["w_edge"] = {k: (np.zeros_like(v) if (k.endswith("_b") and k != "dense_b") else v) for k, v in w.items()}
    return p


STACKED_MISTAKES = ("feedback rows 0..3", "partial k-block dropped", "layer below one step late", "encoder state returned",
                    "head bias of outputs 0..3")


def stacked_decode_reference(w, enc, dec0, L, T_out, act, dt=np.float64, mistake=None):
    """The stacked decode in dtype dt, pre-activations summed as the kernel does (bias, x . K, h . R)
    -> dict(out (B,T_out,O), hT, cT (L,B,H), z_enc [l] (B,T_in,4H), z_dec [l] (B,T_out,4H), pre (B,T_out,O)).
    mistake, one of STACKED_MISTAKES: the decoder's layer 0 contracts only input rows 0..3 of dec0_K; the encoder drops the partial
    last 16-row block of x . enc0_K; a layer l >= 1 reads the layer below at the previous step; with T_out > 0 the returned states
    are the encoder's; the head's outputs 4..7 take the bias of outputs 0..3."""
    assert mistake is None or mistake in STACKED_MISTAKES
    c_ = lambda a: np.asarray(a, dt)
    w = {k: c_(v) for k, v in w.items()}
    enc, dec0 = c_(enc), c_(dec0)
    B, T_in, F = enc.shape
    H, O = w["enc0_R"].shape[0], w["dense_W"].shape[1]
    s = _rec_act(act)
    h, c = [np.zeros((B, H), dt) for _ in range(L)], [np.zeros((B, H), dt) for _ in range(L)]
    late = mistake == "layer below one step late"

    def stack_step(x, side, rows, zs):
        for l in range(L):
            K, R, b = (w["%s%d_%s" % (side, l, k)] for k in "KRb")
            below = h[l - 1] if l else None
            inp = x if l == 0 else (prev_below if late else below)
            prev_below = h[l].copy()                      # this layer's h before its update: what the layer above reads when late
            k_rows = rows if l == 0 else H
            z = (b + inp[:, :k_rows] @ K[:k_rows]) + h[l] @ R
            c[l] = s(z[:, H:2 * H]) * c[l] + s(z[:, :H]) * np.tanh(z[:, 2 * H:3 * H])
            h[l] = s(z[:, 3 * H:]) * np.tanh(c[l])
            zs[l].append(z)

    z_enc, z_dec = [[] for _ in range(L)], [[] for _ in range(L)]
    f_rows = F // 16 * 16 if mistake == "partial k-block dropped" else F
    for t in range(T_in):
        stack_step(enc[:, t], "enc", f_rows, z_enc)
    enc_state = (np.stack(h), np.stack(c))
    bd = w["dense_b"].copy()
    if mistake == "head bias of outputs 0..3":
        bd[4:] = bd[:max(O - 4, 0)]
    o_rows = min(O, 4) if mistake == "feedback rows 0..3" else O
    y, out, pre = dec0[:, 0], [], []
    for _ in range(T_out):
        stack_step(y, "dec", o_rows, z_dec)
        a = h[L - 1] @ w["dense_W"] + bd
        y = np.tanh(a)
        out.append(y); pre.append(a)
    st = lambda v, n: np.stack(v, axis=1) if v else np.zeros((B, 0, n), dt)
    hT, cT = enc_state if (mistake == "encoder state returned" and T_out > 0) else (np.stack(h), np.stack(c))
    return {"out": st(out, O), "hT": hT, "cT": cT, "z_enc": [st(z, 4 * H) for z in z_enc], "z_dec": [st(z, 4 * H) for z in z_dec],
            "pre": st(pre, O)}


RELU_HEAD_BIAS = (0.3, -0.3, 0.1, -0.1, 0.6, -0.6)     # a relu head about half of whose outputs are exactly zero


def regime_selffed(seed, regime, H, O, B, T, dact, residual, dtype=np.float32):
    """The self-fed decoder's inputs with the layer in `regime` (R1 / R2 / R4; it reads a fed-back output: xk = 0.25) -> dict(K, R,
    b, W, bd, x0 (B,O), h0, c0 (B,H; None in R4: the zero state), r (B,O) or None, dloss (T,B,O), act, dact, regime).  The tanh
    head is _regime_head's; the relu head has gain 1 and a bias of both signs."""
    assert regime in ("R1", "R2", "R4") and dact in ("tanh", "relu")
    rng = np.random.default_rng(seed)
    K, R, b = regime_layer(rng, O, H, regime, 0.8, 1.0, None, dtype, xk=0.25)
    if dact == "tanh":
        W, bd = _regime_head(rng, H, O, dtype)
    else:
        W = rng.normal(0.0, 1.0 / np.sqrt(H), (H, O)).astype(dtype)
        bd = np.resize(np.array(RELU_HEAD_BIAS), O).astype(dtype)
    h0, c0 = (None, None) if regime == "R4" else regime_state(rng, B, b, regime, dtype)
    p = {"K": K, "R": R, "b": b, "W": W, "bd": bd, "x0": rng.uniform(-1, 1, (B, O)).astype(dtype), "h0": h0, "c0": c0,
         "r": rng.uniform(-0.5, 0.5, (B, O)).astype(dtype) if residual else None,
         "dloss": rng.standard_normal((T, B, O)).astype(dtype), "act": REGIME_ACT[regime], "dact": dact, "regime": regime}
    return p


def selffed_forward(x0, h0, c0, r, K, R, b, W, bd, T, act, dact, dt=np.float64):
    """fov_selffed_decoder_fwd in dtype dt (z = b + x . K + h . R, this order) -> the tapes in the kernel's layouts: y (B,T,O), Hs,
    Cs (T+1,B,H), XA (T+1,B,O), A (T,B,O), RES (T,B,1,5,H), and the pre-activations z (T,B,4H), pre (T,B,O)."""
    c_ = lambda a: None if a is None else np.asarray(a, dt)
    x, h, c, r, K, R, b, W, bd = (c_(a) for a in (x0, h0, c0, r, K, R, b, W, bd))
    B, O = x.shape
    H = R.shape[0]
    h = np.zeros((B, H), dt) if h is None else h
    c = np.zeros((B, H), dt) if c is None else c
    s = _rec_act(act)
    Hs, Cs, XA, A, RES, zs, pres = [h], [c], [x], [], [], [], []
    for _ in range(T):
        z = (b + x @ K) + h @ R
        i, f, g, o = s(z[:, :H]), s(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), s(z[:, 3 * H:])
        c = f * c + i * g
        h = o * np.tanh(c)
        pre = h @ W + bd
        a = np.tanh(pre) if dact == "tanh" else np.maximum(pre, 0)
        x = a if r is None else a + r
        Hs.append(h); Cs.append(c); XA.append(x); A.append(a); zs.append(z); pres.append(pre)
        RES.append(np.stack([i, f, g, o, c], axis=1)[:, None])
    st = lambda v, shape: np.stack(v).astype(dt) if v else np.zeros(shape, dt)
    XA = np.stack(XA).astype(dt)
    return {"y": np.ascontiguousarray(np.swapaxes(XA[1:], 0, 1)), "Hs": np.stack(Hs).astype(dt), "Cs": np.stack(Cs).astype(dt), "XA": XA,
            "A": st(A, (0, B, O)), "RES": st(RES, (0, B, 1, 5, H)), "z": st(zs, (0, B, 4 * H)), "pre": st(pres, (0, B, O))}


SELFFED_MISTAKES = ("feedback gradient dropped", "c_prev one step late", "tanh derivative from XA", "dc0 without f")


def selffed_backward(tapes, dloss, K, R, W, act, dact, mistake=None):
    """fov_selffed_decoder_bwd written out on GIVEN tapes (Cs, XA, RES and, when the forward had a residual term, A; else a_t =
    XA[t + 1]), in the dtype of dloss: the gate derivative from the stored gate, the relu derivative from a_t > 0, c_{t-1} = Cs[t].
    -> dict(DY, DPRE (T,B,O), DZ (T,B,4H), dx0 (B,O), dh0, dc0 (B,H)).
    mistake, one of SELFFED_MISTAKES: dy_t = dloss_t alone; c_{t-1} read from Cs[t + 1]; a_t of the tanh derivative read from
    XA[1:] although A is given; dc0 without the last multiplication by f."""
    assert mistake is None or mistake in SELFFED_MISTAKES
    dt = dloss.dtype
    c_ = lambda a: np.asarray(a, dt)
    K, R, W, Cs, XA = c_(K), c_(R), c_(W), c_(tapes["Cs"]), c_(tapes["XA"])
    T, B, O = dloss.shape
    H = R.shape[0]
    RES = c_(tapes["RES"]).reshape(T, B, 5, H)
    aout = c_(tapes["A"]) if tapes.get("A") is not None else XA[1:]
    if mistake == "tanh derivative from XA" and dact == "tanh":
        aout = XA[1:]
    DY, DPRE, DZ = np.zeros((T, B, O), dt), np.zeros((T, B, O), dt), np.zeros((T, B, 4 * H), dt)
    dx, dhR, dc = np.zeros((B, O), dt), np.zeros((B, H), dt), np.zeros((B, H), dt)
    for t in range(T - 1, -1, -1):
        dy = dloss[t] if mistake == "feedback gradient dropped" else dloss[t] + dx
        a = aout[t]
        dpre = dy * ((a > 0).astype(dt) if dact == "relu" else (1 - a * a))
        dh = dhR + dpre @ W.T
        i, f, g, o, c = (RES[t, :, q] for q in range(5))
        c_prev = Cs[t + 1] if mistake == "c_prev one step late" else Cs[t]
        tc = np.tanh(c)
        dcv = dc + dh * o * (1 - tc * tc)
        dz = np.concatenate([dcv * g * _rec_act_grad(i, act), dcv * c_prev * _rec_act_grad(f, act), dcv * i * (1 - g * g),
                             dh * tc * _rec_act_grad(o, act)], axis=1)
        dc = dcv if (mistake == "dc0 without f" and t == 0) else dcv * f
        DY[t], DPRE[t], DZ[t] = dy, dpre, dz
        dhR, dx = dz @ R.T, dz @ K.T
    return {"DY": DY, "DPRE": DPRE, "DZ": DZ, "dx0": dx, "dh0": dhR, "dc0": dc}


# --------------------------------------------------------------------------------------
# The tile kernels that train: the self-fed two-layer decoder (fov_selffed2_decoder_fwd / _bwd), the others-mixing decoder at
# H = 32 / 64 (fov_mix_decoder_fwd / _bwd) and the stacked model's training graph (fov_stacked_seq2seq_train_fwd / _bwd) in the
# value regimes above: restatements of the entry points' loops with every tape, the BPTT written out on GIVEN tapes, and
# `mistake`: a named way of being wrong on purpose (finite, plausible), with which the host tests show what the GPU checks see.
# --------------------------------------------------------------------------------------
SELFFED2_STATES = ("h1_0", "c1_0", "h2_0", "c2_0")
SELFFED2_TAPES = ("H1", "C1", "H2", "C2", "XY", "RES1", "RES2")
SELFFED2_GRADS = ("DPRE", "DZ1", "DZ2", "dx0", "dh1_0", "dc1_0", "dh2_0", "dc2_0")
SELFFED2_MISTAKES = ("ctx of step t + 1 at step t", "layer 2 reads h1 of the previous parity", "feedback gradient dropped",
                     "c_prev one step late", "dz2 . K2^T left out of dh1")
TILE_HEAD_BIAS = (12.0, 0.3, -0.3, -12.0, 0.5, -3.0)   # the arguments of a fed-back tanh: a third at least at +-1 (both signs from O = 4
# on), more than a third on the slope, one near -1: at O = 3 .. 6 at least 0.30 of them lie beyond +-9 and 0.30 inside +-1


def _cell(z, c, act, H):
    s = _rec_act(act)
    i, f, g, o = s(z[:, :H]), s(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), s(z[:, 3 * H:])
    c = f * c + i * g
    return o * np.tanh(c), c, np.stack([i, f, g, o, c], 1)


def _gates_bwd(res, c_prev, dh, dc, act):
    """The cell's pointwise backward from the stored (i, f, g, o, c) (B,5,H) -> (dz (B,4H), dc for the step below)."""
    i, f, g, o, c = (res[:, k] for k in range(5))
    tc = np.tanh(c)
    dcv = dc + dh * o * (1 - tc * tc)
    dz = np.concatenate([dcv * g * _rec_act_grad(i, act), dcv * c_prev * _rec_act_grad(f, act), dcv * i * (1 - g * g),
                         dh * tc * _rec_act_grad(o, act)], 1)
    return dz, dcv * f


def selffed2_forward(x0, st, w, T, act, dt=np.float64, mistake=None):
    """fov_selffed2_decoder_fwd's loop in dtype dt (z = b + x . K + h . R; the head bd + h2 . W + ctx_t, in this order) -> (every
    output in the entry point's layout plus z1, z2 (T,B,4H) and pre (T,B,O), the distance of the nearest hard_sigmoid
    pre-activation from +-2.5).  w: dec1_K .. dec2_b, W and, optionally, bd (O,) and ctx (B,T,O); st: SELFFED2_STATES, None = zero.
    mistake: the head of step t takes ctx of step t + 1 (zero behind the last); layer 2 reads h1 of the step before."""
    assert mistake is None or mistake in SELFFED2_MISTAKES
    w = {k: np.asarray(v, dt) for k, v in w.items()}
    B, O_ = x0.shape
    H = w["dec1_R"].shape[0]
    z0 = np.zeros((B, H), dt)
    h1, c1, h2, c2 = (z0 if st.get(k) is None else np.asarray(st[k], dt) for k in SELFFED2_STATES)
    x = np.asarray(x0, dt)
    tp = {"H1": [h1], "C1": [c1], "H2": [h2], "C2": [c2], "XY": [x], "RES1": [], "RES2": [], "z1": [], "z2": [], "pre": []}
    for t in range(T):
        z1 = (w["dec1_b"] + x @ w["dec1_K"]) + h1 @ w["dec1_R"]
        h1_prev = h1
        h1, c1, r1 = _cell(z1, c1, act, H)
        below = h1_prev if mistake == "layer 2 reads h1 of the previous parity" else h1
        z2 = (w["dec2_b"] + below @ w["dec2_K"]) + h2 @ w["dec2_R"]
        h2, c2, r2 = _cell(z2, c2, act, H)
        p = h2 @ w["W"]
        if "bd" in w:
            p = w["bd"] + p
        if "ctx" in w:
            if mistake != "ctx of step t + 1 at step t":
                p = p + w["ctx"][:, t]
            elif t + 1 < T:
                p = p + w["ctx"][:, t + 1]
        x = np.tanh(p)
        for k, v in (("H1", h1), ("C1", c1), ("H2", h2), ("C2", c2), ("XY", x), ("RES1", r1[:, None]), ("RES2", r2[:, None]),
                     ("z1", z1), ("z2", z2), ("pre", p)):
            tp[k].append(v)
    empty = {"RES1": (0, B, 1, 5, H), "RES2": (0, B, 1, 5, H), "z1": (0, B, 4 * H), "z2": (0, B, 4 * H), "pre": (0, B, O_)}
    out = {k: np.stack(v).astype(dt) if v else np.zeros(empty[k], dt) for k, v in tp.items()}
    out["y"] = np.ascontiguousarray(out["XY"][1:].transpose(1, 0, 2))
    out["hT"], out["cT"] = np.stack([h1, h2]).astype(dt), np.stack([c1, c2]).astype(dt)
    margin = np.inf
    if act_code(act) == ACT_HARD_SIGMOID:
        for z in tp["z1"] + tp["z2"]:
            gates = np.concatenate([z[:, :2 * H], z[:, 3 * H:]], 1)
            margin = min(margin, float(np.abs(np.abs(gates) - 2.5).min()))
    return out, margin


def selffed2_backward(tp, dloss, w, act, dt=np.float64, mistake=None):
    """fov_selffed2_decoder_bwd's loop in dtype dt on GIVEN tapes (C1, C2, XY, RES1, RES2) -> SELFFED2_GRADS.
    mistake: dy_t = dloss_t alone; c_{t-1} read from row t + 1 of C1 / C2; dh1 without dz2 . K2^T."""
    assert mistake is None or mistake in SELFFED2_MISTAKES
    w = {k: np.asarray(v, dt) for k, v in w.items()}
    dloss = np.asarray(dloss, dt)
    T, B, O_ = dloss.shape
    H = w["dec1_R"].shape[0]
    tp = {k: np.asarray(tp[k], dtype=dt) for k in ("C1", "C2", "XY", "RES1", "RES2")}
    late = int(mistake == "c_prev one step late")
    out = {"DPRE": np.zeros((T, B, O_), dt), "DZ1": np.zeros((T, B, 4 * H), dt), "DZ2": np.zeros((T, B, 4 * H), dt)}
    dx, dz1, dz2 = np.zeros((B, O_), dt), np.zeros((B, 4 * H), dt), np.zeros((B, 4 * H), dt)
    dc1, dc2 = np.zeros((B, H), dt), np.zeros((B, H), dt)
    for t in range(T - 1, -1, -1):
        y = tp["XY"][t + 1]
        dy = dloss[t] if mistake == "feedback gradient dropped" else dloss[t] + dx
        dpre = dy * (1 - y * y)
        dh2 = dpre @ w["W"].T + dz2 @ w["dec2_R"].T
        dz2, dc2 = _gates_bwd(tp["RES2"][t][:, 0], tp["C2"][t + late], dh2, dc2, act)
        dh1 = dz1 @ w["dec1_R"].T
        if mistake != "dz2 . K2^T left out of dh1":
            dh1 = dz2 @ w["dec2_K"].T + dh1
        dz1, dc1 = _gates_bwd(tp["RES1"][t][:, 0], tp["C1"][t + late], dh1, dc1, act)
        dx = dz1 @ w["dec1_K"].T
        out["DPRE"][t], out["DZ1"][t], out["DZ2"][t] = dpre, dz1, dz2
    out.update(dx0=dx, dh1_0=dz1 @ w["dec1_R"].T, dc1_0=dc1, dh2_0=dz2 @ w["dec2_R"].T, dc2_0=dc2)
    return out


def _two_layer_regime(rng, regime, H, O, B, dtype):
    """Both layers of a self-fed two-layer decoder in `regime`: each reads a computed input (xk = 0.25).  -> (w, states)."""
    w = {}
    w["dec1_K"], w["dec1_R"], w["dec1_b"] = regime_layer(rng, O, H, regime, 0.8, 1.0, None, dtype, xk=0.25)
    w["dec2_K"], w["dec2_R"], w["dec2_b"] = regime_layer(rng, H, H, regime, 0.5, 1.0, None, dtype, xk=0.25)
    if regime == "R4":          # the accumulating regime starts from the zero state
        st = [np.zeros((B, H), dtype) for _ in range(4)]
    else:
        st = list(regime_state(rng, B, w["dec1_b"], regime, dtype) + regime_state(rng, B, w["dec2_b"], regime, dtype))
    return w, st


def regime_selffed2(seed, regime, H, O, B, T, bd=True, dtype=np.float32):
    """The self-fed two-layer decoder's inputs with both layers in `regime` and a saturating head (_regime_head's W; the arguments
    of the fed-back tanh sit at TILE_HEAD_BIAS, on bd + ctx together when bd is given, on ctx alone else)
    -> dict(w (with W, ctx and perhaps bd), x0 (B,O), st {name: (B,H) or None: R4 starts from the zero state}, dloss (T,B,O), act,
    regime).  R3 reaches LAYER 1 AND THE HEAD (regime_mix_decoder's): row 9's first input is +-500, row 3's context is scaled by
    100; extreme = (3, 9), and x0_calm / ctx_calm hold the two rows ordinary."""
    rng = np.random.default_rng(seed)
    w, st = _two_layer_regime(rng, regime, H, O, B, dtype)
    w["W"], bias = _regime_head(rng, H, O, dtype)
    want = np.resize(np.array(TILE_HEAD_BIAS), O)
    ctx = 0.1 * rng.standard_normal((B, T, O))
    if bd:
        w["bd"] = bias
        ctx = ctx + (want - bias.astype(np.float64))
    else:
        ctx = ctx + want
    w["ctx"] = ctx.astype(dtype)
    p = {"w": w, "x0": rng.uniform(-1, 1, (B, O)).astype(dtype), "dloss": rng.standard_normal((T, B, O)).astype(dtype),
         "st": dict(zip(SELFFED2_STATES, [None] * 4 if regime == "R4" else st)), "act": REGIME_ACT[regime], "regime": regime}
    if regime == "R3":
        assert B > 16
        p["extreme"], p["x0_calm"], p["ctx_calm"] = np.array([3, 9]), p["x0"].copy(), w["ctx"].copy()
        w["ctx"][3] *= 100.0
        p["x0"][9] = np.where(p["x0"][9] < 0, -500.0, 500.0)
    return p


MIX_TILE_TAPES = ("M", "P", "H1", "C1", "H2", "C2", "res1", "res2")
MIX_TILE_GRADS = ("DZ1", "DZ2", "dpre_m", "dpre_p", "dh1_0", "dc1_0", "dh2_0", "dc2_0")
MIX_TILE_MISTAKES = ("mix_Wp transposed", "oth_proj of step t + 1 at step t", "dp without 1 - p^2", "feedback gradient dropped",
                     "c_prev one step late")


def mix_tile_forward(dec0, st, oth_proj, w, mix_Wp, T, act, dt=np.float64, mistake=None):
    """mix_decoder_train_forward in dtype dt -> its tapes.  mistake: m_t = tanh(p_t . mix_Wp^T + ..); the mixing tanh of step t
    takes the others' projection of step t + 1 (zero behind the last)."""
    assert mistake is None or mistake in MIX_TILE_MISTAKES
    c_ = lambda a: np.asarray(a, dt)
    Wp, oth = c_(mix_Wp), c_(oth_proj)
    if mistake == "mix_Wp transposed":
        Wp = Wp.T
    if mistake == "oth_proj of step t + 1 at step t":
        oth = np.concatenate([oth[:, 1:], np.zeros_like(oth[:, :1])], axis=1)
    return mix_decoder_train_forward(c_(dec0), *[c_(s) for s in st], oth, {k: c_(v) for k, v in w.items()}, Wp, T, act=act)


def mix_tile_backward(tape, dloss, w, mix_Wp, act, dt=np.float64, mistake=None):
    """mix_decoder_backward in dtype dt on GIVEN tapes (M, P, res1, res2 and C1s, C2s: row t = the cell state BEFORE step t).
    mistake: dpp_t = dm_t . mix_Wp^T without (1 - p_t^2) (P read as zero); dm_t = dloss_t alone (M read as +-1: the feedback term
    vanishes); c_{t-1} read from row t + 1."""
    assert mistake is None or mistake in MIX_TILE_MISTAKES
    c_ = lambda a: np.asarray(a, dt)
    M, P, C1, C2 = c_(tape["M"]), c_(tape["P"]), c_(tape["C1s"]), c_(tape["C2s"])
    if mistake == "dp without 1 - p^2":
        P = np.zeros_like(P)
    if mistake == "feedback gradient dropped":
        M = np.ones_like(M)
    if mistake == "c_prev one step late":
        C1, C2 = (np.concatenate([C[1:T_], c_(tape[r])[T_ - 1:, :, 4]]) for C, r, T_ in ((C1, "res1", M.shape[0]), (C2, "res2", M.shape[0])))
    return mix_decoder_backward(M, P, c_(dloss), c_(tape["res1"]), c_(tape["res2"]), C1, C2, {k: c_(v) for k, v in w.items()}, c_(mix_Wp),
                                act=act)


def regime_mix_tile(seed, regime, H, O, B, T, dtype=np.float32):
    """The others-mixing decoder's inputs at a tile width with both layers in `regime`, _regime_head's Dense head and a mixing
    stage whose arguments sit at TILE_HEAD_BIAS (on the others' projection; mix_Wp at gain 0.15, so the slope outputs stay on the
    slope) -> dict(w, mix_Wp, st [h1, c1, h2, c2] (zeros in R4), dec0 (B,O), oth (B,T,O), G (T,B,O), act, regime).  R3 as
    regime_mix_decoder: row 9's first input is +-500, row 3's projection is scaled by 100; extreme, dec0_calm, oth_calm."""
    rng = np.random.default_rng(seed)
    w, st = _two_layer_regime(rng, regime, H, O, B, dtype)
    w["dense_W"], w["dense_b"] = _regime_head(rng, H, O, dtype)
    p = {"w": w, "mix_Wp": (0.15 * rng.standard_normal((O, O))).astype(dtype), "st": st, "dec0": rng.uniform(-1, 1, (B, O)).astype(dtype),
         "oth": (np.resize(np.array(TILE_HEAD_BIAS), O) + 0.1 * rng.standard_normal((B, T, O))).astype(dtype),
         "G": rng.standard_normal((T, B, O)).astype(dtype), "act": REGIME_ACT[regime], "regime": regime}
    if regime == "R3":
        assert B > 16
        p["extreme"], p["dec0_calm"], p["oth_calm"] = np.array([3, 9]), p["dec0"].copy(), p["oth"].copy()
        p["oth"][3] *= 100.0
        p["dec0"][9] = np.where(p["dec0"][9] < 0, -500.0, 500.0)
    return p


STACKED_TRAIN_TAPES = ("enc_hs", "enc_res", "dec_hs", "dec_res", "hT", "cT")
STACKED_TRAIN_MISTAKES = ("decoder layer l seeded from encoder layer l - 1", "partial k-block dropped", "decoder input rows 0..3",
                          "dx of the layer above dropped", "c_prev one step late", "decoder dc_0 not handed to the encoder")


def stacked_train_forward(w, enc, dec_in, L, act, dt=np.float64, mistake=None):
    """fov_stacked_seq2seq_train_fwd in dtype dt -> dict(enc_hs (L,B,T_in,H), enc_res (L,B,T_in,5,H), dec_hs, dec_res, hT, cT
    (L,B,H), z_enc / z_dec [l] (B,T,4H)).  mistake: decoder layer l starts from encoder layer l - 1's state (layer 0 from the top
    one's); the encoder drops the partial last 16-row block of x . enc0_K; the decoder's layer 0 contracts input rows 0..3 only."""
    assert mistake is None or mistake in STACKED_TRAIN_MISTAKES
    c_ = lambda a: np.asarray(a, dt)
    w = {k: c_(v) for k, v in w.items()}
    enc, dec_in = c_(enc), c_(dec_in)
    F, O = enc.shape[2], dec_in.shape[2]
    f_rows = F // 16 * 16 if mistake == "partial k-block dropped" else F
    o_rows = min(O, 4) if mistake == "decoder input rows 0..3" else O
    out = {k: [] for k in STACKED_TRAIN_TAPES + ("z_enc", "z_dec")}
    x, state = enc[:, :, :f_rows], []
    for l in range(L):
        K, R, b = (w["enc%d_%s" % (l, k)] for k in "KRb")
        K = K[:f_rows] if l == 0 else K
        hs, h, c, res = lstm_layer_train(x, K, R, b, act=act)
        out["enc_hs"].append(hs); out["enc_res"].append(res); out["hT"].append(h); out["cT"].append(c)
        out["z_enc"].append(regime_preactivations(x, K, R, b, hs))
        state.append((h, c))
        x = hs
    x = dec_in[:, :, :o_rows]
    for l in range(L):
        K, R, b = (w["dec%d_%s" % (l, k)] for k in "KRb")
        K = K[:o_rows] if l == 0 else K
        h0, c0 = state[l - 1] if mistake == "decoder layer l seeded from encoder layer l - 1" else state[l]
        hs, _, _, res = lstm_layer_train(x, K, R, b, h0, c0, act=act)
        out["dec_hs"].append(hs); out["dec_res"].append(res)
        out["z_dec"].append(regime_preactivations(x, K, R, b, hs, h0))
        x = hs
    return {k: (np.stack(v) if k in STACKED_TRAIN_TAPES else v) for k, v in out.items()}


def _bptt_from_reserve(res, c0, R, K, din, dh, dc, act, late):
    """One layer's BPTT from its reserve (B,T,5,H): dh_t = din_t + dz_{t+1} . R^T, c_{t-1} = the reserve's c of step t - 1 (c0 at
    t = 0; late: of step t) -> (dz (B,T,4H), dx (B,T,H) or None without K, dh_0, dc_0)."""
    B, T, _, H = res.shape
    dz_all = np.zeros((B, T, 4 * H), res.dtype)
    for t in range(T - 1, -1, -1):
        c_prev = res[:, t, 4] if late else (res[:, t - 1, 4] if t > 0 else c0)
        dz, dc = _gates_bwd(res[:, t], c_prev, dh if din is None else dh + din[:, t], dc, act)
        dz_all[:, t] = dz
        dh = dz @ R.T
    return dz_all, (None if K is None else dz_all @ K.T), dh, dc


def stacked_train_backward(tp, dhs_top, w, L, act, dt=np.float64, mistake=None):
    """fov_stacked_seq2seq_train_bwd in dtype dt on GIVEN tapes (enc_res, dec_res, cT) -> dict(enc_dz (L,B,T_in,4H), dec_dz
    (L,B,T_out,4H)).  mistake: a layer below another gets no dx from it; c_{t-1} read from step t; the decoder's dc_0 does not
    reach the encoder (dh_0 does)."""
    assert mistake is None or mistake in STACKED_TRAIN_MISTAKES
    c_ = lambda a: np.asarray(a, dt)
    w = {k: c_(v) for k, v in w.items()}
    enc_res, dec_res, cT, dhs_top = c_(tp["enc_res"]), c_(tp["dec_res"]), c_(tp["cT"]), c_(dhs_top)
    B, H = cT.shape[1], cT.shape[2]
    late, no_dx = mistake == "c_prev one step late", mistake == "dx of the layer above dropped"
    zero = np.zeros((B, H), dt)
    dec_dz, enc_dz, seed = [None] * L, [None] * L, [None] * L
    din = dhs_top
    for l in range(L - 1, -1, -1):
        dec_dz[l], dx, dh0, dc0 = _bptt_from_reserve(dec_res[l], cT[l], w["dec%d_R" % l], w["dec%d_K" % l] if l else None, din, zero, zero,
                                                     act, late)
        seed[l] = (dh0, zero if mistake == "decoder dc_0 not handed to the encoder" else dc0)
        din = None if no_dx else dx
    din = None
    for l in range(L - 1, -1, -1):
        enc_dz[l], dx, _, _ = _bptt_from_reserve(enc_res[l], zero, w["enc%d_R" % l], w["enc%d_K" % l] if l else None, din, seed[l][0],
                                                 seed[l][1], act, late)
        din = None if no_dx else dx
    return {"enc_dz": np.stack(enc_dz), "dec_dz": np.stack(dec_dz)}
