"""include/fov360.h as a contract, checked call by call on the host with no device.

For every entry point the header says which pointers are required and which may be NULL, which shapes it takes, what an empty
batch does and what a short workspace returns.  This file holds that reading as ONE TABLE (an `E(...)` per entry point) and makes
every call in one child process that sees no device: HIP_VISIBLE_DEVICES and ROCR_VISIBLE_DEVICES are empty in the child's
environment, the child asks the HIP runtime for the device count before its first library call and makes none if a device
answers (the tests then skip with that reason).  Device pointers are made-up addresses, a distinct 256-byte aligned one per
parameter, 1 MiB apart; host-side pointer tables and int arrays are real ctypes arrays.  Without a device a call has one of
three outcomes:

    refused          FOV_ERR_INVALID / _UNSUPPORTED / _WORKSPACE and a message in fov_last_error
    accepted, empty  FOV_OK: the header says the shape launches nothing
    accepted         FOV_ERR_LAUNCH with the runtime's no-device message: the call passed every check and reached a HIP call
                     (a launch, a hipFuncSetAttribute, a zeroing hipMemsetAsync, an epoch re-zero)

so an entry point that touches the device before it has finished validating shows up as `accepted` on a row that expects
`refused`.  Every row is the entry's BASELINE (the smallest supported shape, which must be accepted) with one thing changed:

    a  each required pointer NULL                      refused, FOV_ERR_INVALID (a missing workspace: FOV_ERR_WORKSPACE)
    b  each optional pointer NULL                      accepted; the row cites the header words that make it optional
    c  each size -1 / 0 / one past a documented limit  refused / what the header gives / the code the header names;
       each stride negative, or below the row it strides where the header says so: refused
    d  each enumeration at -1, one past its last value and at every hole: FOV_ERR_INVALID
    e  workspace_bytes = need - 1 / need / NULL workspace / a base 4 bytes off
    f  the alignment rules the header states, the operand 4 bytes off
    g  "before any pointer is looked at": the shape refusal again with EVERY pointer NULL gives the same code
    h  every fov_*_supported predicate against its entry point over the predicate's edges, B > 0, default environment
       (without a device the library counts 256 CUs): 1 = accepted, 0 = FOV_ERR_UNSUPPORTED
    x  rows of one entry point that fit no group (a second mode, a product of sizes, an odd/even rule)

INT_MAX.  A size with a documented bound has its row in c.  For the others INTMAX_ACCEPTED pins every (entry point, argument)
whose INT_MAX still reaches a HIP call; the list is the reading list of the launchers behind them (see the comment there).

Run as `python tests/test_abi_contract_host.py --child OUT.json` the file is the child."""
import ctypes
import itertools
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from longterm360fov_amd import _lib  # noqa: E402

HEADER = os.path.join(ROOT, "include", "fov360.h")
OK, INVALID, UNSUPPORTED, WORKSPACE, LAUNCH = _lib.OK, _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE, _lib.ERR_LAUNCH
REFUSALS = (INVALID, UNSUPPORTED, WORKSPACE)
NO_DEVICE = "no ROCm-capable device"
INT_MAX = 2 ** 31 - 1
FAKE_BASE, FAKE_STEP = 0x7F0000000000, 1 << 20
XCH = 256 + (64 << 20)          # "workspace >= 256 + 64 MB" of the bf16 persistent kernels


def prototypes():
    """name -> [(parameter name, is a pointer, C type)] from the header, parsed as test_abi.py parses it."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    out = {}
    for _, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ \*]*?)\s*\b(fov_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        ps = []
        for p in (q.strip() for q in params.split(",")):
            if p in ("", "void"):
                continue
            words = re.sub(r"[\*]", " ", re.sub(r"\bconst\b", "", p)).split()
            ps.append((words[-1], "*" in p, " ".join(words[:-1])))
        out[name] = ps
    return out


def header_prose():
    """The header's text with comment leaders and line breaks folded away: what a cite must be a substring of."""
    return re.sub(r"\s+", " ", re.sub(r"^\s*\*\s?", "", open(HEADER).read(), flags=re.M))


def _fold(s):
    return re.sub(r"\s+", " ", s).strip()


# Baseline values by parameter name, used where an entry gives none.
DEFAULTS = {"B": 16, "T": 2, "T_in": 2, "T_out": 2, "T1": 2, "T2": 2, "F": 6, "F1": 6, "F2": 6, "F_enc": 6, "F_dec": 6, "H": 64, "O": 6,
            "N": 16, "In": 64, "Out": 6, "M": 16, "K": 64, "n": 96, "rows": 16, "fps": 30, "C": 4, "W": 6, "kh": 3, "kw": 3, "L": 2,
            "act": 0, "impl": 0, "activation": 0, "accumulate": 0}


class E:
    """One entry point's reading of the header.
    base      baseline values of the non-pointer parameters (DEFAULTS for the rest)
    req       required pointers (NULL alone: FOV_ERR_INVALID)
    opt       [(names, cite)]: pointers that may be NULL alone, with the header words that say so
    optgroup  [(names, cite)]: pointers given all or none (all NULL: accepted, one NULL alone: FOV_ERR_INVALID)
    ws        the workspace's size: (size function, its arguments by name or as constants) | bytes | f(values) | None
    ws_names  (pointer, size) parameter names of the workspace
    ws_optional  cite: a NULL workspace is accepted
    ws_misaligned  code of a base 4 bytes off (None: no such row)
    zero      "B:E T:A F:R": the outcome of each size at 0 (E empty, A accepted, R refused); every size is also refused at -1
    limits    [(argument, value, code)]: one past each limit the header states (or a value outside a stated set)
    edges     [(argument, last value taken, code of the next one, step to the next one)]: both sides of a large bound
    enums     {argument: valid values}
    flags     int parameters of which only zero / non-zero matters;  other: int parameters with rows of their own in `extra`
    strides   {argument: smallest value the header allows, or None}: refused negative, and below that value
    align     [(pointer, "refused" | "accepted", cite)]
    pre_ptr   the header says the shape refusal comes before any pointer is looked at
    tables    host-side arrays: {parameter: number of pointers | list of ints}
    extra     [(row name, {argument: value}, (kind, code))]
    accepted  (code, words of the message) of an accepted call; FOV_ERR_LAUNCH with the no-device message unless stated"""

    def __init__(self, name, base=None, req="", opt=(), optgroup=(), ws=None, ws_names=("workspace", "workspace_bytes"),
                 ws_optional=None, ws_misaligned=WORKSPACE, zero="", limits=(), edges=(), enums=None, flags="", other="", strides=None,
                 align=(), pre_ptr=False, tables=None, extra=(), accepted=(LAUNCH, NO_DEVICE)):
        self.name, self.base, self.req = name, dict(base or {}), req.split()
        self.opt = [(n.split(), c) for n, c in opt]
        self.optgroup = [(n.split(), c) for n, c in optgroup]
        self.ws, self.ws_names, self.ws_optional, self.ws_misaligned = ws, ws_names, ws_optional, ws_misaligned
        self.zero = dict(z.split(":") for z in zero.split())
        self.limits, self.enums, self.flags, self.other = list(limits), dict(enums or {}), flags.split(), other.split()
        self.edges = [tuple(g) + (1,) * (4 - len(g)) for g in edges]
        self.strides, self.align, self.pre_ptr = dict(strides or {}), list(align), pre_ptr
        self.tables, self.extra, self.accepted = dict(tables or {}), list(extra), accepted

    def pointers(self):
        """every pointer this entry classifies, required or optional"""
        names = list(self.req) + [n for ns, _ in self.opt + self.optgroup for n in ns]
        if self.ws is not None or self.ws_optional:
            names.append(self.ws_names[0])
        return names

    def integers(self):
        names = list(self.zero) + list(self.enums) + self.flags + self.other + list(self.strides)
        if self.ws is not None or self.ws_optional:
            names.append(self.ws_names[1])
        return names


ACT = {"act": (0, 1)}
ACT_IMPL = {"act": (0, 1), "impl": (0, 1, 2)}
STEPS = 2 ** 29 - 2      # (steps + 2) * ceil(B / 8) <= 2^30 of the persistent-kernel entry points: the last steps taken at B = 16
FUSED = STEPS - 2        # ... of a fused call's T_in or T_out, the other one being the baseline's 2
TILE_B = 2 ** 30         # B, T <= 2^30 of the one-workgroup-per-tile entry points
KH_EDGE = 5592405        # kh kw C N < 2^29 at the conv baseline's kw (or kh) = 3, C = 4, N = 8: the last odd size taken
LSTM_OPT = ("h0 c0 hs hT cT", "h0,c0:(B,H) or NULL (= zeros) hs:(B,T,H) or NULL hT,cT:(B,H) or NULL")
GUARDS = [("guard0 guard1 guard2", "guard0..2 (each may be NULL)"), ("applied", "applied (device pointer, may be NULL)")]
S2S_REQ = "enc_in dec_in0 enc_K enc_R enc_b dec_K dec_R dec_b dense_W dense_b out"
S2S_ZERO = "B:E T_in:A T_out:A F_enc:R F_dec:R H:R"
S2S_WS = ("fov_seq2seq_decode_workspace_bytes", "B T_in T_out F_enc F_dec H impl")
MIXDEC = dict(base={"H": 256, "oth_batch_stride": 12, "oth_step_stride": 6},
              req="dec0 h1 c1 h2 c2 oth_proj dec1_K dec1_R dec1_b dec2_K dec2_R dec2_b dense_W dense_b mix_Wp out",
              opt=[("h1T c1T h2T c2T", "h1T..c2T (B,H): final states or NULL")],
              optgroup=[("P H1 C1 H2 C2 res1 res2", "Training buffers (all or none)")],
              ws=("fov_mix_decoder_workspace_bytes", "B H"), zero="B:E T_out:E H:R O:R", enums=ACT,
              limits=[("H", 128, UNSUPPORTED), ("H", 512, UNSUPPORTED), ("O", 9, UNSUPPORTED)], edges=[("T_out", STEPS, UNSUPPORTED)],
              strides={"oth_batch_stride": None, "oth_step_stride": None})
MIXDEC_BWD = dict(base={"H": 256},
                  req="M P dloss res1 res2 C1 C2 dec1_K dec1_R dec2_K dec2_R dense_W mix_Wp DZ1 DZ2 dpre_m dpre_p dh1_0 dc1_0 dh2_0 dc2_0",
                  ws=("fov_mix_decoder_bwd_workspace_bytes", "B H"), zero="B:E T_out:E H:R O:R", enums=ACT,
                  limits=[("H", 128, UNSUPPORTED), ("H", 512, UNSUPPORTED), ("O", 9, UNSUPPORTED)], edges=[("T_out", STEPS, UNSUPPORTED)])
BWD_OPT = [("h0 c0", "h0/c0 (B,H) or NULL"), ("dhs", "dhs (B,T,H) or NULL"), ("dhT dcT", "dhT/dcT (B,H) or NULL"),
           ("dx", "dx (B,T,F) or NULL"), ("dK dR db", "dK (F,4H), dR (H,4H), db (4H) (each may be NULL)"),
           ("dh0 dc0", "dh0/dc0 (B,H) or NULL")]
LSTM_BWD = dict(req="x K R hs reserve dz", opt=BWD_OPT, ws=("fov_lstm_seq_bwd_workspace_bytes", "B T F H"), zero="B:A T:A F:R H:R",
                enums=ACT, flags="accumulate")
LSTM_BWD_EDGES = [("T", STEPS, UNSUPPORTED)]
DENSE_BWD = dict(req="x W dpre", opt=[("dx dW db", "each output may be NULL")], ws=("fov_dense_bwd_workspace_bytes", "N In Out"),
                 zero="N:A In:R Out:R", flags="accumulate")
CONV = {"B": 2, "H": 6, "W": 6, "C": 4, "N": 8, "kh": 3, "kw": 3, "x_pixel_stride": 4, "x_batch_stride": 144}
CONV_X = {"x_pixel_stride": 4, "x_batch_stride": 144}
CONV_EVEN = [("kh even", {"kh": 2}, ("refused", INVALID)), ("kw even", {"kw": 4}, ("refused", INVALID))]
CELL = {"B": 2, "H": 6, "W": 6, "C": 4, "F": 8, "kh": 3, "kw": 3, "x_pixel_stride": 4, "x_batch_stride": 144,
        "h_prev_pixel_stride": 8, "h_prev_batch_stride": 288, "h_pixel_stride": 8, "recurrent_activation": 0}
CELL_OPT = [("h_prev", "when h_prev is NULL = zero state"), ("b", "b (4F) or NULL"), ("c_prev", "c_prev (B*H*W,F) or NULL"),
            ("gates", "gates (B*H*W,4F) or NULL")]
CELL_STRIDES = {"x_pixel_stride": 4, "x_batch_stride": 144, "h_prev_pixel_stride": 8, "h_prev_batch_stride": 288, "h_pixel_stride": 8}
STATE = dict(base={"workspace_bytes": 4096}, req="workspace", other="workspace_bytes",
             extra=[("workspace_bytes below the 256-byte header", {"workspace_bytes": 255}, ("refused", INVALID))])
STACKED_LIMITS = [("F_enc", 97, UNSUPPORTED), ("F_dec", 9, UNSUPPORTED), ("H", 16, UNSUPPORTED), ("H", 128, UNSUPPORTED),
                  ("L", 1, UNSUPPORTED), ("L", 4, UNSUPPORTED)]
STACKED_EDGES = [("B", TILE_B, UNSUPPORTED), ("T_in", TILE_B, UNSUPPORTED), ("T_out", TILE_B, UNSUPPORTED)]
OPTIM_ZERO = "n:E"

TABLE = [
    E("fov_lstm_seq_fwd", req="x K R b", opt=[LSTM_OPT], ws=("fov_lstm_seq_workspace_bytes", "B T F H impl"),
      zero="B:E T:A F:R H:R", enums=ACT_IMPL, edges=[("T", STEPS, UNSUPPORTED)]),
    E("fov_lstm_seq_fwd_train", req="x K R b reserve", opt=[LSTM_OPT], ws=("fov_lstm_seq_workspace_bytes", "B T F H impl"),
      zero="B:E T:A F:R H:R", enums=ACT_IMPL, edges=[("T", STEPS, UNSUPPORTED)]),
    E("fov_lstm_seq_fwd_zx", req="zx R b", opt=[LSTM_OPT, ("reserve", "(reserve may be NULL)")],
      ws=("fov_lstm_seq_workspace_bytes", "B T 1 H impl"), zero="B:E T:A H:R", enums=ACT_IMPL, edges=[("T", STEPS, UNSUPPORTED)]),
    E("fov_lstm_seq_fwd_bf16", base={"H": 256}, req="x K R b", opt=[LSTM_OPT, ("reserve", "(reserve may be NULL for inference)")],
      ws=XCH, zero="B:E T:A F:R H:R", enums=ACT, limits=[("F", 257, UNSUPPORTED), ("H", 128, UNSUPPORTED), ("H", 512, UNSUPPORTED)], edges=[("T", STEPS, UNSUPPORTED)]),
    E("fov_dense_fwd", req="x W y", opt=[("b", "b may be NULL (no bias)")], zero="N:E In:R Out:R", enums={"activation": (0, 1)},
      edges=[("In", 2 ** 24, INVALID), ("Out", 2 ** 24, INVALID)]),
    E("fov_dense_add_fwd", base={"add_row_stride": 6}, req="x W add y", opt=[("b", "(0 broadcasts one row); b may be NULL")], zero="N:E In:R Out:R",
      enums={"activation": (0, 1)}, strides={"add_row_stride": None}, edges=[("In", 2 ** 24, INVALID), ("Out", 2 ** 24, INVALID)]),
    E("fov_dense_fwd_bf16", req="x W y", opt=[("b", "b may be NULL")], zero="N:E In:R Out:R", enums={"activation": (0, 1)},
      limits=[("In", 257, UNSUPPORTED), ("Out", 17, UNSUPPORTED)]),
    E("fov_mix_head_fwd", base={"add_row_stride": 6}, req="h dense_W dense_b mix_Wp add p m", zero="N:E H:R O:R",
      limits=[("O", 9, INVALID), ("H", 2052, INVALID), ("H", 66, INVALID)], strides={"add_row_stride": None},
      align=[("h", "refused", "h 16-byte aligned")]),
    E("fov_mix_head_bwd", req="dm_loss m p mix_Wp dense_W dpre_m dpre_p dh", opt=[("dm_feedback", "(NULL at the last step)")],
      zero="N:E H:R O:R", limits=[("O", 9, INVALID)]),
    E("fov_mix_head_wgrad", base={"n_others": 3}, req="h2 dpre_p others p dpre_m out",
      ws=("fov_mix_head_wgrad_workspace_bytes", "B T_out H O n_others"), zero="B:A T_out:A H:R O:R n_others:A", flags="accumulate",
      limits=[("O", 9, INVALID)],
      extra=[("others NULL with n_others = 0", {"others": None, "n_others": 0}, ("accepted", None))]),
    E("fov_mix_decoder_fwd", **MIXDEC),
    E("fov_mix_decoder_fwd_bf16", **MIXDEC),
    E("fov_mix_decoder_bwd", **MIXDEC_BWD),
    E("fov_mix_decoder_bwd_bf16", **MIXDEC_BWD),
    E("fov_mix_decoder_prepack", base={"H": 256, "fwd_bytes": ("fov_mix_decoder_workspace_bytes", "1 256"),
                                       "bwd_bytes": ("fov_mix_decoder_bwd_workspace_bytes", "1 256")},
      req="dec2_K", opt=[("workspace_fwd workspace_bwd", "(either may be NULL)")], other="fwd_bytes bwd_bytes H",
      extra=[("H = 128", {"H": 128}, ("refused", INVALID)), ("H = 0", {"H": 0}, ("refused", INVALID)),
             ("fwd_bytes = need - 1", {"fwd_bytes": -1}, ("refused", WORKSPACE)),
             ("bwd_bytes = need - 1", {"bwd_bytes": -1}, ("refused", WORKSPACE)),
             ("both workspaces NULL: nothing to pack", {"workspace_fwd": None, "workspace_bwd": None}, ("empty", None))]),
    E("fov_seq2seq_decode_fwd_bf16", base={"H": 256}, req=S2S_REQ, opt=[("hT cT", "hT / cT (B,H) or NULL")], ws=XCH, zero=S2S_ZERO,
      enums=ACT, limits=[("F_enc", 257, UNSUPPORTED), ("F_dec", 9, UNSUPPORTED), ("H", 128, UNSUPPORTED), ("H", 512, UNSUPPORTED)],
      edges=[("T_in", FUSED, UNSUPPORTED), ("T_out", FUSED, UNSUPPORTED)]),
    E("fov_seq2seq_decode_fwd", req=S2S_REQ, opt=[("hT cT", "hT,cT: final decoder state (B,H) or NULL")], ws=S2S_WS, zero=S2S_ZERO,
      enums=ACT_IMPL, limits=[("F_dec", 65, UNSUPPORTED)], edges=[("T_in", FUSED, UNSUPPORTED), ("T_out", FUSED, UNSUPPORTED)]),
    E("fov_seq2seq_decode_fwd_packed", req=S2S_REQ,
      opt=[("hT cT", "hT,cT: final decoder state (B,H) or NULL"), ("enc_Rpack dec_Rpack", "either may be NULL")], ws=S2S_WS,
      zero=S2S_ZERO, enums=ACT_IMPL, limits=[("F_dec", 65, UNSUPPORTED)],
      edges=[("T_in", FUSED, UNSUPPORTED), ("T_out", FUSED, UNSUPPORTED)],
      align=[("enc_Rpack", "refused", "A pack that is not 16-byte aligned is FOV_ERR_INVALID"),
             ("dec_Rpack", "refused", "A pack that is not 16-byte aligned is FOV_ERR_INVALID")]),
    E("fov_seq2seq_decoder_fwd", req="dec_in0 dec_K dec_R dec_b dense_W dense_b out",
      opt=[("h0 c0", "(h0, c0) (B,H) (NULL = zeros)"), ("hT cT", "hT, cT (B,H) optional final state")],
      ws=("fov_seq2seq_decode_workspace_bytes", "B 0 T_out 1 F_dec H impl"), zero="B:E T_out:E F_dec:R H:R", enums=ACT_IMPL,
      limits=[("F_dec", 65, UNSUPPORTED)], edges=[("T_out", STEPS, UNSUPPORTED)]),
    E("fov_seq2seq_tf_fwd", req="enc_in dec_in enc_K enc_R enc_b dec_K dec_R dec_b dense_W out",
      opt=[("dense_b", "dense_b may be NULL")], ws=("fov_seq2seq_tf_workspace_bytes", "B T_in T_out F_enc F_dec H impl"),
      zero=S2S_ZERO, enums=ACT_IMPL,
      edges=[("T_in", STEPS, UNSUPPORTED), ("T_out", (2 ** 31 - 1) // 16, UNSUPPORTED)]),      # T_out: B * T_out <= INT_MAX binds first
    E("fov_lstm_pack_r", req="R out", zero="H:R", limits=[("H", 32, UNSUPPORTED), ("H", 512, UNSUPPORTED)],
      align=[("out", "refused", "out: H * 4H floats, 16-byte aligned"), ("R", "accepted", "R needs no alignment beyond a float's")]),
    E("fov_stacked_seq2seq_decode_fwd",
      req="enc_in dec_in0 enc0_K enc0_R enc0_b enc1_K enc1_R enc1_b dec0_K dec0_R dec0_b dec1_K dec1_R dec1_b dense_W dense_b out",
      opt=[("enc2_K enc2_R enc2_b dec2_K dec2_R dec2_b", "the third layer's six pointers are NULL (and ignored) for L = 2"),
           ("hT cT", "hT, cT (L,B,H) or NULL")],
      zero="B:E T_in:A T_out:A F_enc:R F_dec:R H:R L:R", enums=ACT, limits=STACKED_LIMITS, edges=STACKED_EDGES,
      extra=[("L = 3 without its third layer", {"L": 3, "enc2_R": None}, ("refused", INVALID))]),
    E("fov_selffed_decoder_fwd", base={"dact": 1}, req="x0 K R b W bd",
      optgroup=[("h0 c0", "both NULL = the zero state")],
      opt=[("r", "the residual link's term of :103-107, or NULL"), ("Hs Cs XA A RES y", "Outputs, each of which may be NULL and is then not written")],
      zero="B:E T:E O:R H:R", enums={"act": (0, 1), "dact": (1, 2)},
      limits=[("O", 9, UNSUPPORTED), ("H", 16, UNSUPPORTED), ("H", 128, UNSUPPORTED)],
      edges=[("B", TILE_B, UNSUPPORTED), ("T", TILE_B, UNSUPPORTED)]),
    E("fov_selffed_decoder_bwd", base={"dact": 1, "a_from_A": 0}, req="Cs XA RES dloss K R W DY DPRE DZ dx0",
      opt=[("dh0 dc0", "either may be NULL"), ("A", "a_t is read from A when a_from_A != 0, else from XA[1:]")],
      zero="B:E T:A O:R H:R", enums={"act": (0, 1), "dact": (1, 2)}, flags="a_from_A",
      limits=[("O", 9, UNSUPPORTED), ("H", 16, UNSUPPORTED), ("H", 128, UNSUPPORTED)],
      edges=[("B", TILE_B, UNSUPPORTED), ("T", TILE_B, UNSUPPORTED)],
      extra=[("A NULL with a_from_A = 1", {"A": None, "a_from_A": 1}, ("refused", INVALID)),
             ("XA NULL with a_from_A = 1", {"XA": None, "a_from_A": 1}, ("accepted", None))]),
    E("fov_selffed2_decoder_fwd", req="x0 K1 R1 b1 K2 R2 b2 W",
      opt=[("h1_0 c1_0 h2_0 c2_0", "each may be NULL = zeros"), ("bd ctx", "bd (O) and ctx (B,T,O) are each optional"),
           ("H1 C1 H2 C2 XY RES1 RES2 y hT cT", "Outputs, each of which may be NULL and is then not written")],
      zero="B:E T:E O:R H:R", enums=ACT, limits=[("O", 9, UNSUPPORTED), ("H", 16, UNSUPPORTED), ("H", 128, UNSUPPORTED)],
      edges=[("B", TILE_B, UNSUPPORTED), ("T", TILE_B, UNSUPPORTED)],
      pre_ptr=True),
    E("fov_selffed2_decoder_bwd", base={"H": 32}, req="C1 C2 XY RES1 RES2 dloss K1 R1 K2 R2 W DPRE DZ1 DZ2",
      opt=[("dx0 dh1_0 dc1_0 dh2_0 dc2_0", "each of these five optional")], zero="B:E T:A O:R H:R", enums=ACT,
      limits=[("O", 9, UNSUPPORTED), ("H", 16, UNSUPPORTED), ("H", 64, UNSUPPORTED)],
      edges=[("B", TILE_B, UNSUPPORTED), ("T", TILE_B, UNSUPPORTED)], pre_ptr=True),
    E("fov_stacked_seq2seq_train_fwd", req="enc_in dec_in enc_K enc_R enc_b dec_K dec_R dec_b",
      opt=[("enc_hs enc_res dec_hs dec_res dec_top hT cT", "Outputs, each of which may be NULL and is then not written")],
      tables={k: 4 for k in "enc_K enc_R enc_b dec_K dec_R dec_b".split()},
      zero="B:E T_in:A T_out:A F_enc:R F_dec:R H:R L:R", enums=ACT, limits=STACKED_LIMITS, edges=STACKED_EDGES, pre_ptr=True),
    E("fov_stacked_seq2seq_train_bwd", req="enc_res dec_res cT dhs_top enc_R enc_K dec_R dec_K enc_dz dec_dz",
      tables={k: 4 for k in "enc_R enc_K dec_R dec_K".split()}, ws_names=("scratch", "scratch_bytes"),
      ws=("fov_stacked_seq2seq_train_bwd_scratch_bytes", "B T_in T_out H"), zero="B:E T_in:A T_out:A H:R L:R", enums=ACT,
      limits=STACKED_LIMITS[2:], edges=STACKED_EDGES, pre_ptr=True),
    E("fov_meanvar_xyz", req="y out", zero="rows:E fps:R", edges=[("fps", 2 ** 20, INVALID)]),
    E("fov_lstm_seq_bwd", edges=LSTM_BWD_EDGES, **LSTM_BWD),
    E("fov_lstm_seq_bwd_bf16", base={"H": 256}, limits=[("H", 128, INVALID)], edges=LSTM_BWD_EDGES,
      align=[("R", "refused", "R must be 16-byte aligned (else FOV_ERR_INVALID)"), ("K", "accepted", "fp32 when K is not aligned")],
      **LSTM_BWD),
    E("fov_dense_bwd", **DENSE_BWD),
    E("fov_dense_bwd_bf16", **DENSE_BWD),
    E("fov_lstm_seq_wgrad", base={"bf16": 0}, req="x hs dz", opt=[("h0", "zero when h0 is NULL"), ("dK dR db", "Any of dK / dR / db may be NULL")],
      ws=("fov_lstm_seq_bwd_workspace_bytes", "B T F H"), zero="B:A T:A F:R H:R", flags="accumulate bf16",
      extra=[("bf16 operands at H = 64", {"bf16": 1}, ("refused", INVALID)),
             ("x NULL without dK", {"x": None, "dK": None}, ("accepted", None))]),
    E("fov_lstm_seq_wgrad_pair", req="x1 hs1 dz1 x2 hs2 dz2",
      opt=[("h0_1 h0_2", "zero when h0 is NULL"), ("dK1 dR1 db1 dK2 dR2 db2", "Any of dK / dR / db may be NULL")],
      ws=("fov_lstm_seq_bwd_workspace_bytes", "B T1 F1 H"), zero="B:A T1:A T2:A F1:R F2:R H:R", flags="accumulate"),
    E("fov_lstm_seq_wgrad_layers", req="x F T hs h0 dz dK dR db",
      tables={"x": 4, "hs": 4, "h0": 4, "dz": 4, "dK": 4, "dR": 4, "db": 4, "F": [6, 6, 6, 6], "T": [2, 2, 2, 2]},
      ws=("fov_lstm_seq_bwd_workspace_bytes", "B 2 6 H"), zero="B:A H:R L:R", flags="accumulate",
      limits=[("L", 5, UNSUPPORTED)]),
    E("fov_wgrad_fused", base={"In1": 64, "In2": 64, "bias": 1, "bf16": 0}, req="x1 x2 dpre out",
      ws=("fov_wgrad_fused_workspace_bytes", "N In1 In2 Out"), zero="In1:R In2:A N:A Out:R", flags="bias accumulate bf16",
      extra=[("x2 NULL with In2 = 0", {"x2": None, "In2": 0}, ("accepted", None)),
             ("N past INT_MAX", {"N": 2 ** 31}, ("refused", INVALID))]),
    E("fov_mse_dense_grad", req="y target dpre", opt=[("loss", "(loss may be NULL)")],
      ws=lambda v: 4 * ((v["n"] + 255) // 256 + 64), zero="n:E", enums={"activation": (0, 1)}),
    E("fov_mse_dense_grad_w", base={"weight": 1.0, "time_major_B": 0, "time_major_T": 0, "O": 0}, req="y target dpre",
      opt=[("loss", "(loss may be NULL)")], ws=lambda v: 4 * ((v["n"] + 255) // 256 + 64), zero="n:E",
      enums={"activation": (0, 1)}, other="time_major_B time_major_T O",
      extra=[("time-major, n = B T O", {"time_major_B": 8, "time_major_T": 2, "O": 6}, ("accepted", None)),
             ("time-major, n != B T O", {"time_major_B": 8, "time_major_T": 2, "O": 5}, ("refused", INVALID)),
             ("time-major, B = 0", {"time_major_B": 0, "time_major_T": 2, "O": 6}, ("refused", INVALID))]),
    E("fov_mse_dense_grad_db", base={"weight": 1.0}, req="y target dpre db", opt=[("loss", "(loss may be NULL)")],
      ws=lambda v: 4 * (9 * ((v["n"] + 255) // 256) + 64 + 256 * max(v["O"], 0)), zero="n:A O:R", enums={"activation": (0, 1)},
      extra=[("n no multiple of O", {"n": 97}, ("refused", INVALID))]),
    E("fov_dense_mse_head", base={"weight": 1.0}, req="hs W b target dW db", opt=[("y", "(may be NULL)"), ("dX", "dloss/dhs (may be NULL)"),
                                                                                   ("loss", "mean (y - target)^2 (may be NULL)")],
      ws=("fov_dense_mse_head_workspace_bytes", "N H O"), zero="N:E H:R O:R", enums={"activation": (0, 1)},
      limits=[("N", 2 ** 20 + 1, UNSUPPORTED), ("H", 516, UNSUPPORTED), ("H", 66, UNSUPPORTED), ("O", 9, UNSUPPORTED)],
      accepted=(UNSUPPORTED, "no ticket slot")),      # the loss ticket needs a device: beyond it nothing is decidable here
    E("fov_scale", req="x", base={"s": 0.5}, zero="n:E"),
    E("fov_act_fwd", req="x y", zero="n:E", enums={"activation": (0, 1, 2, 3)}),
    E("fov_act_bwd", req="dy y out", opt=[("base", "base may be NULL")], zero="n:E", enums={"activation": (0, 1, 2, 3)}),
    E("fov_gauss_nll_grad", base={"T_y": 2}, req="mu var y dmu dvar", opt=[("loss", "*loss (may be NULL)")],
      ws=lambda v: 4 * (max(v["B"], 0) + 64), zero="B:E T_y:R fps:R",
      edges=[("B", 2 ** 29, INVALID), ("T_y", (2 ** 31 - 1) // 90, INVALID), ("fps", (2 ** 31 - 1) // 6, INVALID)]),
    E("fov_rmsprop_tf_step", base={"n": 16}, req="params grads ms", zero=OPTIM_ZERO),
    E("fov_rmsprop_tf_step_guarded", base={"n": 16}, req="params grads ms", opt=GUARDS, zero=OPTIM_ZERO),
    E("fov_adam_step", base={"n": 16, "step": 1}, req="params grads m v", zero=OPTIM_ZERO, other="step",
      extra=[("step = 0", {"step": 0}, ("refused", INVALID)), ("step = -1", {"step": -1}, ("refused", INVALID))]),
    E("fov_adam_step_guarded", base={"n": 16, "step": 1}, req="params grads m v", opt=GUARDS, zero=OPTIM_ZERO, other="step",
      extra=[("step = 0", {"step": 0}, ("refused", INVALID))]),
    E("fov_rmsprop_step", base={"n": 16}, req="params grads accum", zero=OPTIM_ZERO),
    E("fov_rmsprop_step_guarded", base={"n": 16}, req="params grads accum", opt=GUARDS, zero=OPTIM_ZERO),
    E("fov_guard_flag", req="out", opt=[("guard0 guard1 guard2", "guard0..2: each may be NULL, as for the optimizers")]),
    E("fov_tf_head_fwd", base={"M": 32, "O": 3}, req="h mu_W1 mu_b1 mu_W2 mu_b2 var_W1 var_b1 var_W2 var_b2 a1 mu a3 var",
      zero="B:E H:R M:R O:R",
      limits=[("B", 65, UNSUPPORTED), ("H", 2049, UNSUPPORTED), ("M", 33, UNSUPPORTED), ("O", 9, UNSUPPORTED)]),
    E("fov_tf_head_bwd", base={"M": 32, "O": 3},
      req="h mu_W1 mu_W2 var_W1 var_W2 a1 mu a3 var dmu dvar g_mu_W1 g_mu_b1 g_mu_W2 g_mu_b2 g_var_W1 g_var_b1 g_var_W2 g_var_b2 dh",
      zero="B:A H:R M:R O:R", flags="accumulate",
      limits=[("B", 65, UNSUPPORTED), ("H", 2049, UNSUPPORTED), ("M", 33, UNSUPPORTED), ("O", 9, UNSUPPORTED)]),
    E("fov_mlp_head_fwd", base={"final_mode": 1, "n_mix": 4}, req="x W b acts dims act_codes", opt=[("masks", "masks (array or NULL)")],
      tables={"W": 4, "b": 4, "masks": 4, "acts": 4, "dims": [64, 32, 40, 1, 1], "act_codes": [2, 0, 0, 0]},
      zero="B:E L:R n_mix:R", enums={"final_mode": (0, 1)}, limits=[("L", 5, UNSUPPORTED), ("n_mix", 33, INVALID)],
      extra=[("dims[0] = 2049", {"dims": [2049, 32, 40, 1, 1]}, ("refused", UNSUPPORTED)),
             ("dims[1] = 513", {"dims": [64, 513, 40, 1, 1]}, ("refused", UNSUPPORTED)),
             ("dims[1] = 0", {"dims": [64, 0, 40, 1, 1]}, ("refused", UNSUPPORTED)),
             ("last layer not 10 n_mix wide", {"dims": [64, 32, 41, 1, 1]}, ("refused", INVALID)),
             ("a layer's pointer NULL inside W", {"W": "4 null@1"}, ("refused", INVALID))]),
    E("fov_mlp_head_bwd", req="x W acts dlast gW gb dims act_codes", opt=[("masks", "masks (array or NULL)"), ("dx", "if dx != NULL")],
      tables={"W": 4, "masks": 4, "acts": 4, "gW": 4, "gb": 4, "dims": [64, 32, 40, 1, 1], "act_codes": [2, 0, 0, 0]},
      ws=lambda v: 4 * (v["B"] * 32 + 64), ws_misaligned=None, zero="B:A L:R", flags="accumulate", limits=[("L", 5, UNSUPPORTED)],
      extra=[("dims[0] = 2049", {"dims": [2049, 32, 40, 1, 1]}, ("refused", UNSUPPORTED)),
             ("a layer's pointer NULL inside gW", {"gW": "4 null@1"}, ("refused", INVALID))]),
    E("fov_gmm3d_loss_grad", base={"n_mix": 4, "n_pts": 30, "ldy": 90, "scale": 1.0, "weight_by_pi": 0}, req="params y dpre",
      opt=[("loss", "*loss (may be NULL: gradient only)")], ws=lambda v: 256 + 4 * v["B"], ws_misaligned=None, zero="B:E n_mix:R n_pts:R", flags="weight_by_pi",
      limits=[("n_mix", 33, UNSUPPORTED), ("n_pts", 257, UNSUPPORTED)], strides={"ldy": 90}),
    E("fov_gmm3d_sample", base={"n_mix": 4, "n_pts": 30, "ldo": 90}, req="params u z out", zero="B:E n_mix:R n_pts:R",
      limits=[("n_mix", 33, UNSUPPORTED)], strides={"ldo": 90}),
    E("fov_categorical_crossentropy_grad", base={"n_pix": 648, "C": 30}, req="p target dp", opt=[("loss", "*loss (may be NULL)")],
      ws=lambda v: 4 * (v["n_pix"] // 256 + 65), zero="n_pix:E C:R"),
    E("fov_xyz_sum1_grad", base={"n_pix": 648, "C": 30}, req="p dp", opt=[("reg", "*reg (may be NULL)")],
      ws=lambda v: 4 * (v["n_pix"] // 256 + 65), zero="n_pix:E C:R", limits=[("C", 2, INVALID)]),
    E("fov_sample_refeed_fwd", base={"ldx": 90, "std_mode": 0, "layout": 0}, req="mu var noise x", zero="B:E fps:R",
      enums={"std_mode": (0, 1), "layout": (0, 1)}, strides={"ldx": 90}, edges=[("B", 2 ** 29, INVALID)],
      extra=[("fps = 2^20, the last value taken", {"fps": 2 ** 20, "ldx": 3 * 2 ** 20}, ("accepted", None)),
             ("fps = 2^20 + 1", {"fps": 2 ** 20 + 1, "ldx": 3 * 2 ** 20 + 3}, ("refused", INVALID))]),
    E("fov_sample_refeed_bwd", base={"ldx": 90, "std_mode": 0, "layout": 0}, req="dx var noise dmu dvar", zero="B:E fps:R",
      enums={"std_mode": (0, 1), "layout": (0, 1)}, flags="accumulate", strides={"ldx": 90}, edges=[("B", 2 ** 29, INVALID)],
      extra=[("fps = 2^20, the last value taken", {"fps": 2 ** 20, "ldx": 3 * 2 ** 20}, ("accepted", None)),
             ("fps = 2^20 + 1", {"fps": 2 ** 20 + 1, "ldx": 3 * 2 ** 20 + 3}, ("refused", INVALID))]),
    E("fov_lstm_stack2_fwd", base={"H": 512}, req="x K1 R1 b1 K2 R2 b2",
      opt=[("h0_1 c0_1 h0_2 c0_2", "h0_* / c0_* (B,H) or NULL"), ("reserve1 reserve2", "reserve* (B,T,5,H) or NULL"),
           ("hs1", "hs1 may be NULL"), ("hs2 hT1 cT1 hT2 cT2", "hs2, hT* and cT* may be NULL")],
      ws=XCH, zero="B:E T:R F:R H:R", enums=ACT,
      limits=[("B", 65, UNSUPPORTED), ("T", 1, UNSUPPORTED), ("F", 97, UNSUPPORTED), ("H", 256, UNSUPPORTED), ("H", 1024, UNSUPPORTED)]),
    E("fov_lstm_stack2_fwd_bf16", base={"H": 256}, req="x K1 R1 b1 K2 R2 b2",
      opt=[("hs1 hT1 cT1 reserve1 hs2 hT2 cT2 reserve2", "hs / hT / cT / reserve of either layer may be NULL")],
      ws=XCH, zero="B:E T:R F:R H:R", enums=ACT,
      limits=[("B", 513, UNSUPPORTED), ("T", 1, UNSUPPORTED), ("F", 97, UNSUPPORTED), ("H", 128, UNSUPPORTED), ("H", 512, UNSUPPORTED)]),
    E("fov_lstm_stack2_bwd", base={"H": 512}, req="x R1 K2 R2 hs1 reserve1 hs2 reserve2 dz1 dz2",
      opt=[("h0_1 c0_1 h0_2 c0_2", "h0_* / c0_* (B,H) or NULL"),
           ("dhs2 dhT2 dcT2 dhT1 dcT1", "dhs2 (B,T,H) / dhT2 / dcT2 / dhT1 / dcT1 optional upstream gradients"),
           ("dK1 dR1 db1 dK2 dR2 db2", "dK / dR / db of either layer optional"), ("dh0_1 dc0_1 dh0_2 dc0_2", "dh0 / dc0 optional")],
      ws=("fov_lstm_stack2_bwd_workspace_bytes", "B T F H"), zero="B:A T:A F:R H:R", enums=ACT, flags="accumulate",
      limits=[("B", 33, UNSUPPORTED), ("H", 256, UNSUPPORTED), ("H", 1024, UNSUPPORTED)],
      extra=[("empty batch at a width the kernel does not have", {"B": 0, "H": 128}, ("refused", UNSUPPORTED)),
             ("no steps at a width the kernel does not have", {"T": 0, "H": 128}, ("refused", UNSUPPORTED))]),
    E("fov_matmul", req="a b c", ws=("fov_matmul_workspace_bytes", "M K N"), ws_optional="The workspace is optional (NULL allowed)",
      zero="M:E K:A N:E"),
    E("fov_conv2d_fwd", base=CONV, req="x w y", opt=[("b add", "b, add (B,H,W,N) may be NULL")], zero="B:E H:R W:R C:R N:R kh:R kw:R",
      enums={"activation": (0, 2)}, strides=CONV_X, extra=CONV_EVEN),
    E("fov_conv2d_dilated_fwd", base=dict(CONV, dilation=2), req="x w y", opt=[("b add", "b, add (B,H,W,N) may be NULL")],
      zero="B:E H:R W:R C:R N:R kh:R kw:R dilation:R", enums={"activation": (0, 2)}, strides=CONV_X, extra=CONV_EVEN),
    E("fov_conv2d_fwd2", base={"B": 2, "H": 6, "W": 6, "C1": 4, "C2": 4, "N": 8, "x1_pixel_stride": 4, "x1_batch_stride": 144,
                               "x2_pixel_stride": 4, "x2_batch_stride": 144},
      req="x1 x2 w y", opt=[("b add", "b, add (B,H,W,N) may be NULL")], zero="B:E H:R W:R C1:R C2:R N:R kh:R kw:R",
      enums={"activation": (0, 2)}, extra=CONV_EVEN,
      strides={"x1_pixel_stride": 4, "x1_batch_stride": 144, "x2_pixel_stride": 4, "x2_batch_stride": 144}),
    E("fov_conv2d_pack_bf16", base=CONV, req="w packed", zero="C:R N:R kh:R kw:R", extra=CONV_EVEN,
      align=[("packed", "refused", "(16-byte aligned, caller-owned device memory)")]),
    E("fov_conv2d_fwd_bf16", base=CONV, req="x w_packed y", opt=[("b", "b, y, B .. activation as in fov_conv2d_fwd")],
      zero="B:E H:R W:R C:R N:R kh:R kw:R", enums={"activation": (0, 2)}, strides=CONV_X, extra=CONV_EVEN,
      align=[("w_packed", "refused", "(16-byte aligned, caller-owned device memory)")]),
    E("fov_convlstm_cell_fwd", base=CELL, req="x w c_new h", opt=CELL_OPT, zero="B:E H:R W:R C:R F:R kh:R kw:R",
      enums={"recurrent_activation": (0, 1)}, strides=CELL_STRIDES, extra=CONV_EVEN),
    E("fov_convlstm_cell_dilated_fwd", base=dict(CELL, dilation=2), req="x w c_new h", opt=CELL_OPT,
      zero="B:E H:R W:R C:R F:R kh:R kw:R dilation:R", enums={"recurrent_activation": (0, 1)}, strides=CELL_STRIDES, extra=CONV_EVEN),
    E("fov_convlstm_cell_pack_bf16", base={"Ctot": 12, "F": 8}, req="w packed", zero="Ctot:R F:R kh:R kw:R", extra=CONV_EVEN,
      align=[("packed", "refused", "(16-byte aligned, caller-owned device memory)")]),
    E("fov_convlstm_cell_fwd_bf16", base=CELL, req="x w_packed c_new h", opt=CELL_OPT, zero="B:E H:R W:R C:R F:R kh:R kw:R",
      enums={"recurrent_activation": (0, 1)}, strides=CELL_STRIDES, extra=CONV_EVEN,
      align=[("w_packed", "refused", "(16-byte aligned, caller-owned device memory)")]),
    E("fov_convlstm_gates", base={"F": 8, "h_pixel_stride": 8}, req="z c h", zero="rows:E F:R", enums=ACT, strides={"h_pixel_stride": 8}),
    E("fov_convlstm_gates_train", base={"F": 8, "h_pixel_stride": 8}, req="z c_new h gates",
      opt=[("c_prev", "(c_prev may be NULL = zero state)")], zero="rows:E F:R", enums=ACT, strides={"h_pixel_stride": 8}),
    E("fov_convlstm_gates_bwd", base={"F": 8, "dh_pixel_stride": 8}, req="dh dc gates c_new dz", opt=[("c_prev", "c_prev (NULL = zero)")],
      zero="rows:E F:R", enums=ACT, strides={"dh_pixel_stride": 8}),
    E("fov_softmax_lastdim", base={"n": 30}, req="x y", zero="rows:E n:R"),
    E("fov_softmax_lastdim_bwd", base={"n": 30}, req="dp p dy", zero="rows:E n:R"),
    E("fov_conv2d_wgrad", base=dict(CONV, x_batch_stride=None), req="x dy dw", ws=("fov_conv2d_wgrad_workspace_bytes", "C N kh kw"),
      ws_optional="without a workspace (NULL) or with a smaller one the product is split less or not at all",
      zero="B:A H:R W:R C:R N:R kh:R kw:R", flags="accumulate", strides={"x_pixel_stride": 4},
      edges=[("kh", KH_EDGE, UNSUPPORTED, 2), ("kw", KH_EDGE, UNSUPPORTED, 2)],
      extra=CONV_EVEN + [("accumulate without a workspace", {"accumulate": 1, "workspace": None}, ("refused", WORKSPACE)),
                         ("accumulate with less than kh kw C N floats", {"accumulate": 1, "workspace_bytes": 4 * 3 * 3 * 4 * 8 - 4},
                          ("refused", WORKSPACE)),
                         ("accumulate with kh kw C N floats", {"accumulate": 1, "workspace_bytes": 4 * 3 * 3 * 4 * 8}, ("accepted", None))]),
    E("fov_conv2d_dilated_wgrad", base=dict(CONV, x_batch_stride=None, dilation=2), req="x dy dw",
      ws=("fov_conv2d_wgrad_workspace_bytes", "C N kh kw"),
      ws_optional="without a workspace (NULL) or with a smaller one the product is split less or not at all",
      zero="B:A H:R W:R C:R N:R kh:R kw:R dilation:R", flags="accumulate", strides={"x_pixel_stride": 4}, extra=CONV_EVEN,
      edges=[("kh", KH_EDGE, UNSUPPORTED, 2), ("kw", KH_EDGE, UNSUPPORTED, 2)]),
    E("fov_conv2d_wgrad_bf16", base=dict(CONV, x_batch_stride=None, dy_row_stride=8), req="x dy dw",
      ws=("fov_conv2d_wgrad_bf16_workspace_bytes", "C N kh kw"), zero="B:A H:R W:R C:R N:R kh:R kw:R", flags="accumulate",
      strides={"x_pixel_stride": 4, "dy_row_stride": 8}, extra=CONV_EVEN),
    E("fov_conv2d_weight_transpose", base={"N": 8}, req="w wt", zero="kh:R kw:R C:R N:R"),
    E("fov_colsum", base={"cols": 8}, req="x out", ws=lambda v: 4 * (256 * max(v["cols"], 0) + 64), zero="rows:A cols:R", flags="accumulate",
      edges=[("cols", 2 ** 24, INVALID)]),
    E("fov_window_stacks", base={"U": 4, "S": 40, "feat": 6, "T": 10, "stride": 1, "collapse_user": 1}, req="x enc fut fut_in",
      zero="U:E S:E feat:R T:R stride:R", flags="collapse_user",
      extra=[("stride > T", {"stride": 11}, ("refused", INVALID)), ("S < 2 T: no window", {"S": 19}, ("empty", None))]),
    E("fov_window_inputs", base={"rows": 64, "n": 8, "n_pairs": 4, "n_others": 3, "fut_offset": 2, "enc_width": 6},
      req="secs feat sample others_base", opt=[("enc dec_in target others future_raw", "Outputs, contiguous, any of them NULL (not written)")],
      zero="rows:A fps:R n:E n_pairs:A n_others:A T_in:R T_out:R fut_offset:A", other="enc_width",
      extra=[("enc_width = 3 fps", {"enc_width": 90}, ("accepted", None)), ("enc_width = 7", {"enc_width": 7}, ("refused", INVALID)),
             ("enc_width = 7 without enc", {"enc_width": 7, "enc": None}, ("accepted", None)),
             ("others_base NULL with n_others = 0", {"others_base": None, "n_others": 0}, ("accepted", None)),
             ("every output NULL: nothing to write", {k: None for k in "enc dec_in target others future_raw".split()}, ("empty", None))]),
    E("fov_fov_hit_rate", base={"pred_row_stride": 3, "gt_row_stride": 3, "span_deg": 100.0, "gt_span_deg": 100.0}, req="pred_xyz gt_xyz out",
      zero="rows:E", strides={"pred_row_stride": 3, "gt_row_stride": 3}),
    E("fov_onehot_maps", base={"xyz_seq_stride": 180, "xyz_step_stride": 90, "maps_seq_stride": 2 * 36 * 18 * 32, "maps_step_stride": 36 * 18 * 32,
                               "channels": 32, "N": 4, "T": 2, "theta_index": None, "phi_index": None},
      req="xyz status", optgroup=[("theta_out phi_out", "both or neither")],
      opt=[("maps", "maps may be NULL when theta_out / phi_out"), ("theta_index phi_index", "Pass xyz = NULL for the second form")],
      zero="N:E T:E", enums={"channels": (30, 32)},
      strides={"xyz_seq_stride": None, "xyz_step_stride": None, "maps_seq_stride": None, "maps_step_stride": None},
      align=[("maps", "refused", "base 16-byte aligned")],
      extra=[("the index form", {"xyz": None, "theta_index": 1, "phi_index": 1}, ("accepted", None)),
             ("xyz and the index arrays", {"theta_index": 1, "phi_index": 1}, ("refused", INVALID)),
             ("one index array alone", {"xyz": None, "theta_index": 1}, ("refused", INVALID)),
             ("neither maps nor index outputs", {"maps": None, "theta_out": None, "phi_out": None}, ("refused", INVALID)),
             ("a maps stride that is no multiple of 4", {"maps_step_stride": 36 * 18 * 32 + 2}, ("refused", INVALID)),
             ("N T past INT_MAX", {"N": INT_MAX, "T": 2}, ("refused", INVALID))]),
    E("fov_heatmap_argmax", base={"map_stride": 648 * 30, "pixel_stride": 30, "out_stride": 30, "n_maps": 4, "n_pix": 648, "C": 30},
      req="maps index", opt=[("value", "(value may be NULL)")], zero="n_maps:E n_pix:R C:R",
      limits=[("C", 65, INVALID), ("n_pix", 2 ** 20 + 1, INVALID)], strides={"map_stride": None, "pixel_stride": 30, "out_stride": 30}),
    E("fov_heatmap_index_xyz", base={"n": 16}, req="index xyz status", zero="n:E"),
    E("fov_categorical_accuracy", base={"pred_s0": 960, "pred_s1": 480, "pred_row_stride": 30, "tgt_s0": 480, "tgt_s1": 960, "tgt_row_stride": 30,
                                        "n0": 2, "n1": 2, "rows": 16, "C": 30},
      req="pred target matches", zero="n0:A n1:A rows:A C:R", flags="accumulate",
      strides={"pred_s0": None, "pred_s1": None, "pred_row_stride": 30, "tgt_s0": None, "tgt_s1": None, "tgt_row_stride": 30},
      align=[("matches", "refused", "*matches (device memory, 8-byte aligned)")],
      extra=[("more than 2^40 rows", {"n0": 2 ** 20, "n1": 2 ** 20, "rows": 2}, ("refused", INVALID)),
             ("pred NULL under accumulate", {"pred": None, "accumulate": 1}, ("refused", INVALID)),
             ("operands NULL over an empty shape", {"pred": None, "target": None, "rows": 0}, ("accepted", None)),
             ("an empty shape under accumulate", {"rows": 0, "accumulate": 1}, ("empty", None))]),
    E("fov_workspace_init", **STATE),
    E("fov_workspace_force_safe", **dict(STATE, flags="on")),
    E("fov_debug_set_epoch", **dict(STATE, base={"workspace_bytes": 4096, "epoch": 5}, other="workspace_bytes epoch")),
    E("fov_exchange_mode", **STATE),
]
TABLE_BY_NAME = {e.name: e for e in TABLE}

# int-returning entry points with a pointer parameter that have no table entry, each with its reason (twelve at most)
EXCLUDED = {
    "fov_stream_create": "creates a HIP stream: nothing to decide without a device beyond its NULL check",
    "fov_stream_destroy": "destroys a HIP stream: needs one",
    "fov_check_status": "copies the status header from the device and synchronises",
    "fov_onehot_status": "copies the status word from the device and synchronises",
}
# decided on the host alone (no call of theirs reaches the device here): rows of their own, host_rows() below
HOST_ONLY = ("fov_reduce_defer_begin", "fov_reduce_defer_flush", "fov_reduce_defer_end", "fov_mlp_head_supported")

# "entry point argument" of every size whose INT_MAX is ACCEPTED (reaches a HIP call) where the header states no bound.  The list
# is pinned so that a new one shows up here and is read.  What the launchers behind these do with the value:
#   64-bit element counts, grid = (count + 255) / 256 in long, rows indexed as long * int width, int loops over the width:
#     fov_scale, fov_act_fwd / _bwd, the six optimizer steps, fov_mse_dense_grad(_w), fov_categorical_crossentropy_grad n_pix / C,
#     fov_xyz_sum1_grad, fov_meanvar_xyz rows, fov_fov_hit_rate, fov_heatmap_index_xyz, fov_convlstm_gates(_train, _bwd) rows,
#     fov_softmax_lastdim(_bwd) rows / n, fov_mix_head_bwd (N * H), fov_conv2d_weight_transpose and fov_window_stacks (one long
#     product of all four), fov_colsum rows (long, at most 256 chunks);
#   capped or overflow-checked: fov_mix_head_fwd N and the 16-row form of fov_dense(_add)_fwd N (2048 blocks), fov_heatmap_argmax
#     n_maps (65536 blocks), fov_categorical_accuracy and fov_window_inputs (__builtin_mul_overflow, then capped);
#   a block per row with size_t row offsets, 2^31 - 1 being the grid's own limit: fov_gmm3d_loss_grad / _sample B;
#   tile counts that were int and are long now: the wave-per-row form of fov_dense(_add)_fwd N, fov_dense_fwd_bf16 N,
#     fov_mlp_head_fwd / _bwd B;
#   int index arithmetic inside the kernel, now bounded by the entry point (rows of group c, both sides of each bound):
#     fov_meanvar_xyz fps (3 * f), fov_gauss_nll_grad B / T_y / fps (3 * b, 3 T_y fps), fov_sample_refeed_fwd / _bwd B / fps,
#     fov_colsum cols ((cols + 255) / 256), fov_dense(_add)_fwd In / Out (k += 64);
#   NOT READ, all of them behind a GEMM or an implicit-GEMM convolution: fov_lstm_seq_fwd(_train) H and fov_seq2seq_tf_fwd
#     F_dec / H (the step-wise form), fov_lstm_seq_bwd(_bf16) F, fov_lstm_stack2_bwd F, fov_lstm_seq_wgrad(_pair, _layers) B / T,
#     fov_wgrad_fused In2 / N, fov_dense_bwd(_bf16) N, fov_mix_head_wgrad B / T_out, fov_matmul M, dilation of the two dilated
#     forwards, fov_conv2d_fwd_bf16 N, B / H / W / dilation of the three conv weight gradients.
INTMAX_ACCEPTED = """
fov_act_bwd n
fov_act_fwd n
fov_adam_step n
fov_adam_step_guarded n
fov_categorical_accuracy n0
fov_categorical_accuracy n1
fov_categorical_accuracy rows
fov_categorical_crossentropy_grad C
fov_categorical_crossentropy_grad n_pix
fov_colsum rows
fov_conv2d_dilated_fwd dilation
fov_conv2d_dilated_wgrad B
fov_conv2d_dilated_wgrad H
fov_conv2d_dilated_wgrad W
fov_conv2d_dilated_wgrad dilation
fov_conv2d_fwd_bf16 N
fov_conv2d_weight_transpose C
fov_conv2d_weight_transpose N
fov_conv2d_weight_transpose kh
fov_conv2d_weight_transpose kw
fov_conv2d_wgrad H
fov_conv2d_wgrad W
fov_conv2d_wgrad_bf16 H
fov_conv2d_wgrad_bf16 W
fov_convlstm_cell_dilated_fwd dilation
fov_convlstm_gates rows
fov_convlstm_gates_bwd rows
fov_convlstm_gates_train rows
fov_dense_add_fwd N
fov_dense_bwd N
fov_dense_bwd_bf16 N
fov_dense_fwd N
fov_dense_fwd_bf16 N
fov_fov_hit_rate rows
fov_gmm3d_loss_grad B
fov_gmm3d_sample B
fov_heatmap_argmax n_maps
fov_heatmap_index_xyz n
fov_lstm_seq_bwd F
fov_lstm_seq_bwd_bf16 F
fov_lstm_seq_fwd H
fov_lstm_seq_fwd_train H
fov_lstm_seq_wgrad B
fov_lstm_seq_wgrad T
fov_lstm_seq_wgrad_layers B
fov_lstm_seq_wgrad_pair B
fov_lstm_seq_wgrad_pair T1
fov_lstm_seq_wgrad_pair T2
fov_lstm_stack2_bwd F
fov_matmul M
fov_meanvar_xyz rows
fov_mix_head_bwd H
fov_mix_head_bwd N
fov_mix_head_fwd N
fov_mix_head_wgrad B
fov_mix_head_wgrad T_out
fov_mlp_head_bwd B
fov_mlp_head_fwd B
fov_mse_dense_grad n
fov_mse_dense_grad_w n
fov_rmsprop_step n
fov_rmsprop_step_guarded n
fov_rmsprop_tf_step n
fov_rmsprop_tf_step_guarded n
fov_scale n
fov_seq2seq_tf_fwd F_dec
fov_seq2seq_tf_fwd H
fov_softmax_lastdim n
fov_softmax_lastdim rows
fov_softmax_lastdim_bwd n
fov_softmax_lastdim_bwd rows
fov_wgrad_fused In2
fov_wgrad_fused N
fov_window_inputs n
fov_window_inputs n_pairs
fov_window_inputs rows
fov_window_stacks S
fov_window_stacks T
fov_window_stacks U
fov_window_stacks feat
fov_xyz_sum1_grad n_pix
"""

# ------------------------------------------------------------------------------------------------------------------------ child


class Caller:
    """Builds argument lists from an entry's baseline and records every call."""

    def __init__(self, out_rows):
        self.L = _lib.lib()
        self.protos = prototypes()
        self.rows = out_rows
        self.keep = []          # ctypes arrays stay alive until the process ends

    def _array(self, k, spec):
        if isinstance(spec, (int, str)):    # a table of made-up device addresses; "4 null@1": entry 1 of the 4 is NULL
            n, hole = (spec, -1) if isinstance(spec, int) else (int(spec.split()[0]), int(spec.split("@")[1]))
            arr = (ctypes.c_void_p * n)(*[None if j == hole else FAKE_BASE + (k + 1) * FAKE_STEP + 0x1000 * (j + 1) for j in range(n)])
        else:
            arr = (ctypes.c_int * len(spec))(*spec)
        self.keep.append(arr)
        return ctypes.cast(arr, ctypes.c_void_p).value

    def size_of(self, spec, vals):
        if spec is None:
            return 0
        if isinstance(spec, int):
            return spec
        if callable(spec):
            return spec(vals)
        fn, names = spec
        return int(getattr(self.L, fn)(*[vals[a] if a in vals else int(a) for a in names.split()]))

    def args(self, e, changes=None, ws_delta=0):
        """The baseline with `changes` applied; sizes of workspaces follow the changed shape unless a change names them."""
        changes = dict(changes or {})
        ps = self.protos[e.name]
        vals = {}
        for k, (nm, ptr, ctype) in enumerate(ps):
            if nm == "stream":
                vals[nm] = None
            elif ptr:
                if nm in e.tables:
                    spec = changes.pop(nm) if isinstance(changes.get(nm), (list, str)) else e.tables[nm]
                    vals[nm] = self._array(k, spec)
                elif nm in e.base:
                    vals[nm] = e.base[nm]
                else:
                    vals[nm] = FAKE_BASE + (k + 1) * FAKE_STEP
            elif ctype in ("float", "double"):
                vals[nm] = e.base.get(nm, 0.5)
            elif nm == e.ws_names[1] and (e.ws is not None or e.ws_optional):
                vals[nm] = None                                  # below
            elif isinstance(e.base.get(nm), tuple):
                vals[nm] = None                                  # a size function: below
            else:
                vals[nm] = e.base[nm] if nm in e.base else (0 if nm in e.flags and nm not in DEFAULTS else DEFAULTS[nm])
        offsets = {}
        for nm, v in changes.items():
            if isinstance(v, str) and v.startswith("+"):        # a pointer moved by so many bytes
                offsets[nm] = int(v[1:])
            elif v == 1 and any(nm == p[0] and p[1] for p in ps):    # a pointer the baseline leaves NULL, given
                vals[nm] = FAKE_BASE + ([p[0] for p in ps].index(nm) + 1) * FAKE_STEP
            elif isinstance(e.base.get(nm), tuple):
                vals[nm] = self.size_of(e.base[nm], vals) + v    # relative to the size function's answer
            else:
                vals[nm] = v
        for nm in vals:
            if vals[nm] is None and isinstance(e.base.get(nm), tuple):
                vals[nm] = self.size_of(e.base[nm], vals)
        if e.ws is not None or e.ws_optional:
            if vals[e.ws_names[1]] is None:
                vals[e.ws_names[1]] = max(self.size_of(e.ws, vals) + ws_delta, 0)
        for nm, d in offsets.items():
            vals[nm] += d
        return [vals[nm] for nm, _, _ in ps]

    def call(self, e, group, row, expect, changes=None, ws_delta=0, null_all=False):
        print("ROW %s | %s | %s" % (e.name, group, row), flush=True)
        a = self.args(e, changes, ws_delta)
        if null_all:
            a = [None if p[1] else v for p, v in zip(self.protos[e.name], a)]
        rc = int(getattr(self.L, e.name)(*a))
        err = (self.L.fov_last_error() or b"").decode("utf-8", "replace")
        self.rows.append({"entry": e.name, "group": group, "row": row, "expect": list(expect), "rc": rc, "err": err[:200],
                          "accept": list(e.accepted)})
        return rc


ZERO_KIND = {"E": "empty", "A": "accepted", "R": "refused"}


def entry_rows(c, e):
    ps = c.protos[e.name]
    wp, wb = e.ws_names
    has_ws = e.ws is not None or e.ws_optional
    c.call(e, "baseline", "baseline", ("accepted", None))
    for p in e.req:
        c.call(e, "a", "%s = NULL" % p, ("refused", INVALID), {p: None})
    for names, _ in e.opt:
        for p in names:
            c.call(e, "b", "%s = NULL" % p, ("accepted", None), {p: None})
    for names, _ in e.optgroup:
        c.call(e, "b", "%s all NULL" % " ".join(names), ("accepted", None), {p: None for p in names})
        for p in names:
            c.call(e, "a", "%s = NULL alone" % p, ("refused", INVALID), {p: None})
    for nm, z in e.zero.items():
        c.call(e, "c", "%s = -1" % nm, ("refused", None), {nm: -1})
        c.call(e, "c", "%s = 0" % nm, (ZERO_KIND[z], None), {nm: 0})
    for nm, v, code in e.limits:
        c.call(e, "c", "%s = %d" % (nm, v), ("refused", code), {nm: v})
        if e.pre_ptr:
            c.call(e, "g", "%s = %d with every pointer NULL" % (nm, v), ("refused", code), {nm: v}, null_all=True)
    for nm, last, code, step in e.edges:
        c.call(e, "c", "%s = %d, the last value taken" % (nm, last), ("accepted", None), {nm: last})
        c.call(e, "c", "%s = %d" % (nm, last + step), ("refused", code), {nm: last + step})
        if e.pre_ptr:
            c.call(e, "g", "%s = %d with every pointer NULL" % (nm, last + step), ("refused", code), {nm: last + step}, null_all=True)
    for nm, least in e.strides.items():
        c.call(e, "c", "%s = -1" % nm, ("refused", None), {nm: -1})
        if least is not None:
            c.call(e, "c", "%s = %d, below the row" % (nm, least - 1), ("refused", None), {nm: least - 1})
    for nm, valid in e.enums.items():
        for v in [min(valid) - 1, max(valid) + 1] + [h for h in range(min(valid), max(valid)) if h not in valid]:
            c.call(e, "d", "%s = %d" % (nm, v), ("refused", INVALID), {nm: v})
        for v in valid:
            c.call(e, "d", "%s = %d" % (nm, v), ("accepted", None), {nm: v})
    if has_ws:
        short = ("accepted", None) if e.ws_optional else ("refused", WORKSPACE)
        c.call(e, "e", "%s = need - 1" % wb, short, ws_delta=-1)
        c.call(e, "e", "%s = need" % wb, ("accepted", None))
        c.call(e, "e", "%s = NULL" % wp, short, {wp: None})
        if e.ws_misaligned is not None:
            c.call(e, "e", "%s 4 bytes off" % wp, ("refused", e.ws_misaligned), {wp: "+4"}, ws_delta=16)
    for p, kind, _ in e.align:
        c.call(e, "f", "%s 4 bytes off" % p, (kind, INVALID if kind == "refused" else None), {p: "+4"})
    for row, changes, expect in e.extra:
        c.call(e, "x", row, expect, changes)
    # INT_MAX of every size without a row past a stated limit: recorded, judged against the pinned list
    limited = {nm for nm, v, _ in e.limits if v > 1} | {g[0] for g in e.edges}
    for nm in e.zero:
        if nm not in limited:
            c.call(e, "intmax", nm, ("any", None), {nm: INT_MAX})


def _grid(**axes):
    names = list(axes)
    return [dict(zip(names, v)) for v in itertools.product(*axes.values())]


def _one_at_a_time(base, **axes):
    out = []
    for nm, values in axes.items():
        out += [dict(base, **{nm: v}) for v in values]
    return out


def predicate_rows(c):
    L = c.L

    def check(pred, pargs, entry, changes, tag):
        sup = int(getattr(L, pred)(*pargs))
        e = TABLE_BY_NAME[entry]
        expect = ("accepted_or_empty", None) if sup == 1 else ("refused", UNSUPPORTED)
        c.call(e, "h", "%s%s = %d: %s" % (pred, tuple(pargs), sup, tag), expect, changes)

    for g in _grid(B=(1, 17), T=(0, 1), O=(1, 8, 9), H=(16, 32, 64, 128)):
        a = (g["B"], g["T"], g["O"], g["H"])
        check("fov_selffed_decoder_supported", a, "fov_selffed_decoder_fwd", g, "forward")
        check("fov_selffed_decoder_supported", a, "fov_selffed_decoder_bwd", g, "backward")
        check("fov_selffed2_decoder_supported", a + (0,), "fov_selffed2_decoder_fwd", g, "forward")
        check("fov_selffed2_decoder_supported", a + (1,), "fov_selffed2_decoder_bwd", g, "backward")
    stacked = _grid(F_enc=(1, 96, 97), F_dec=(1, 8, 9), H=(16, 32, 64, 128), L=(1, 2, 3, 4))
    stacked += _one_at_a_time({"F_enc": 6, "F_dec": 6, "H": 32, "L": 3}, B=(1, 17), T_in=(0, 1), T_out=(0, 1))
    for g in stacked:
        g = dict({"B": 16, "T_in": 2, "T_out": 2}, **g)
        a = tuple(g[k] for k in "B T_in T_out F_enc F_dec H L".split())
        check("fov_stacked_seq2seq_decode_supported", a, "fov_stacked_seq2seq_decode_fwd", g, "decode")
        check("fov_stacked_seq2seq_train_supported", a, "fov_stacked_seq2seq_train_fwd", g, "train forward")
        if g["F_enc"] == 6 or (g["F_enc"], g["F_dec"]) == (1, 1):
            b = {k: g[k] for k in "B T_in T_out H L".split()}
            check("fov_stacked_seq2seq_train_supported", a[:3] + (1, 1) + a[5:], "fov_stacked_seq2seq_train_bwd", b, "train backward")
    for g in _grid(B=(1, 64, 65), T=(1, 2, 3), F=(1, 96, 97), H=(256, 512, 1024)):
        check("fov_lstm_stack2_supported", tuple(g.values()), "fov_lstm_stack2_fwd", g, "fp32")
    for g in _grid(B=(1, 512, 513), T=(1, 2, 3), F=(1, 96, 97), H=(128, 256, 512)):
        check("fov_lstm_stack2_supported_bf16", tuple(g.values()), "fov_lstm_stack2_fwd_bf16", g, "bf16")
    for g in _grid(B=(1, 32, 33), T=(1, 2, 100000), F=(1, 97), H=(256, 512, 1024)):
        check("fov_lstm_stack2_bwd_supported", tuple(g.values()), "fov_lstm_stack2_bwd", g, "backward")
    for g in _grid(B=(1, 64, 65), H=(1, 2048, 2049), M=(1, 32, 33), O=(1, 8, 9)):
        check("fov_tf_head_supported", tuple(g.values()), "fov_tf_head_fwd", g, "forward")
        check("fov_tf_head_supported", tuple(g.values()), "fov_tf_head_bwd", g, "backward")
    for g in _grid(N=(1, 2 ** 20, 2 ** 20 + 1), H=(4, 6, 512, 516), O=(1, 8, 9)):
        check("fov_dense_mse_head_supported", tuple(g.values()), "fov_dense_mse_head", g, "head")
    for B, Lr, d0, d1 in itertools.product((1, 16), (1, 2, 4, 5), (1, 2048, 2049), (1, 512, 513)):
        dims = ([d0] + [d1] * (Lr - 1) + [40] + [1] * 4)[:6]
        arr = (ctypes.c_int * len(dims))(*dims)
        sup = int(L.fov_mlp_head_supported(B, Lr, arr))
        expect = ("accepted_or_empty", None) if sup == 1 else ("refused", UNSUPPORTED)
        tag = "fov_mlp_head_supported(%d, %d, %s) = %d" % (B, Lr, dims[:Lr + 1], sup)
        c.call(TABLE_BY_NAME["fov_mlp_head_fwd"], "h", tag + ": forward", expect, {"B": B, "L": Lr, "dims": dims})
        bwd = TABLE_BY_NAME["fov_mlp_head_bwd"]
        need = 4 * (B * sum(dims[1:Lr]) + 64) if sup else 0
        c.call(bwd, "h", tag + ": backward", expect, {"B": B, "L": Lr, "dims": dims, "workspace_bytes": need})
    # one launch or two calls: both are accepted, the predicate only says which
    for g in _grid(B=(1, 32, 33), T1=(1, 20, 21), T2=(1, 20), H=(64, 256, 512)):
        sup = int(L.fov_lstm_seq_wgrad_pair_one_launch(g["B"], g["T1"], g["T2"], g["H"]))
        c.call(TABLE_BY_NAME["fov_lstm_seq_wgrad_pair"], "h", "fov_lstm_seq_wgrad_pair_one_launch%s = %d" % (tuple(g.values()), sup),
               ("accepted", None), dict(g, workspace_bytes=1 << 40))
    # fov_cluster_supported says where impl = cluster has the cluster kernel; where it says 0 the wide kernels may still take the
    # layer under impl = cluster (H = 512, or F > 96 at H = 256), so only the 1 is a claim about the entry point
    for F, H in itertools.product((1, 96, 97), (32, 64, 128, 256, 512)):
        if int(L.fov_cluster_supported(F, H)) == 1:
            c.call(TABLE_BY_NAME["fov_lstm_seq_fwd"], "h", "fov_cluster_supported(%d, %d) = 1" % (F, H), ("accepted", None),
                   {"F": F, "H": H, "impl": _lib.IMPL_CLUSTER})


def host_rows(c):
    """The deferral registry's contract and the one predicate that takes a pointer: FOV_OK here means host bookkeeping only."""
    L = c.L
    base, arena = FAKE_BASE, FAKE_BASE + (1 << 30)

    def row(entry, name, expect, *a):
        print("ROW %s | x | %s" % (entry, name), flush=True)
        rc = int(getattr(L, entry)(*a))
        err = (L.fov_last_error() or b"").decode("utf-8", "replace")
        c.rows.append({"entry": entry, "group": "x", "row": name, "expect": list(expect), "rc": rc, "err": err[:200],
                       "accept": [LAUNCH, NO_DEVICE]})

    begin, flush, end = "fov_reduce_defer_begin", "fov_reduce_defer_flush", "fov_reduce_defer_end"
    row(begin, "grad_base = NULL opens nothing", ("empty", None), None, 1024, arena, 1 << 20, None)
    row(begin, "arena = NULL", ("refused", INVALID), base, 1024, None, 1 << 20, None)
    row(begin, "arena_bytes = 255", ("refused", INVALID), base, 1024, arena, 255, None)
    row(begin, "arena_bytes = 256", ("empty", None), base, 1024, arena, 256, None)
    for i in range(1, 16):
        row(begin, "region %d" % (i + 1), ("empty", None), base + i * 4096, 1024, arena, 1 << 20, None)
    row(begin, "a 17th open region", ("refused", UNSUPPORTED), base + 16 * 4096, 1024, arena, 1 << 20, None)
    row(flush, "an address inside a region, nothing pending", ("empty", None), base + 3 * 4096 + 8, None)
    row(flush, "grad_base = NULL: every region", ("empty", None), None, None)
    row(end, "one region", ("empty", None), base + 3 * 4096, None)
    row(begin, "a slot is free again", ("empty", None), base + 16 * 4096, 1024, arena, 1 << 20, None)
    row(end, "grad_base = NULL: every region", ("empty", None), None, None)
    dims = (ctypes.c_int * 3)(64, 32, 40)
    row("fov_mlp_head_supported", "dims = NULL", ("value", 0), 16, 2, None)
    row("fov_mlp_head_supported", "two layers", ("value", 1), 16, 2, dims)
    row("fov_mlp_head_supported", "B = 0", ("value", 0), 0, 2, dims)


def device_count():
    """(hipError_t, count) of hipGetDeviceCount on the runtime the library links."""
    _lib.lib()                                                # loads the library and, with it, its HIP runtime; no HIP call
    path = None
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            path = line.split()[-1]
            break
    if path is None:
        return None, None
    n = ctypes.c_int(-1)
    rc = ctypes.CDLL(path).hipGetDeviceCount(ctypes.byref(n))
    return int(rc), int(n.value)


def child(out_path):
    t0 = time.time()
    result = {"rows": [], "skipped": None, "error": None}
    rc, n = device_count()
    if rc is None:      # the project's own plumbing, not missing hardware: the parent fails on it, nothing skips
        result["error"] = "the HIP runtime of the library was not found among the process's mappings"
    elif not ((rc == 0 and n == 0) or rc == 100):             # hipSuccess with no device, or hipErrorNoDevice
        result["skipped"] = "a device is visible to the child (hipGetDeviceCount: error %d, %d devices): no call was made" % (rc, n)
    else:
        c = Caller(result["rows"])
        for e in TABLE:
            entry_rows(c, e)
        predicate_rows(c)
        host_rows(c)
    result["seconds"] = time.time() - t0
    result["modules"] = sorted(m for m in sys.modules if m.split(".")[0] in ("torch", "numpy") or m == "longterm360fov_amd.ops")
    with open(out_path, "w") as f:
        json.dump(result, f)
    print("DONE", flush=True)


# ----------------------------------------------------------------------------------------------------------------------- parent

_RESULT = {}


def result():
    """The child's outcomes; the child runs once per session."""
    if _RESULT:
        return _RESULT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    t0 = time.time()
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "rows.json")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], env=env, cwd=ROOT, capture_output=True,
                           text=True, timeout=600)
        lines = p.stdout.strip().splitlines()
        _RESULT["returncode"] = p.returncode
        _RESULT["last"] = lines[-1] if lines else ""
        _RESULT["stderr"] = p.stderr[-2000:]
        _RESULT["data"] = json.load(open(out)) if os.path.exists(out) else None
    _RESULT["wall"] = time.time() - t0
    return _RESULT


def rows(group=None):
    import pytest
    r = result()
    assert r["returncode"] == 0 and r["data"] is not None, \
        "the child ended with status %s in or after [%s]\n%s" % (r["returncode"], r["last"], r["stderr"])
    assert not r["data"]["error"], r["data"]["error"]
    if r["data"]["skipped"]:
        pytest.skip(r["data"]["skipped"])
    return [x for x in r["data"]["rows"] if group is None or x["group"] == group]


def judge(x):
    """None if the row came out as expected, else what is wrong with it."""
    kind, code = x["expect"]
    acc_rc, acc_words = x["accept"]
    accepted = x["rc"] == acc_rc and acc_words in x["err"]
    if kind == "any":
        return None
    if kind == "value":
        return None if x["rc"] == code else "expected %d" % code
    if kind == "accepted":
        return None if accepted else "expected accepted"
    if kind == "empty":
        return None if x["rc"] == OK else "expected FOV_OK with nothing launched"
    if kind == "accepted_or_empty":
        return None if accepted or x["rc"] == OK else "expected accepted"
    assert kind == "refused", kind
    if accepted:
        return "expected a refusal, the call reached the device"
    if code is None:
        return None if x["rc"] in REFUSALS and x["err"] else "expected a refusal"
    return None if x["rc"] == code and x["err"] else "expected error %d" % code


def _wrong(group):
    bad = []
    for x in rows(group):
        why = judge(x)
        if why:
            bad.append("%s [%s] %s: %s, got %d (%s)" % (x["entry"], x["group"], x["row"], why, x["rc"], x["err"][:90]))
    return bad


def _int_entry_points():
    return [n for n, (res, args) in _lib.SIGNATURES.items()
            if res is ctypes.c_int and any(a is ctypes.c_void_p or (isinstance(a, type) and issubclass(a, ctypes._Pointer)) for a in args)]


def test_every_entry_point_is_tabled_or_excluded_by_name():
    names = _int_entry_points()
    assert len(EXCLUDED) <= 12 and all(EXCLUDED.values())
    assert not set(EXCLUDED) & set(TABLE_BY_NAME) and not set(HOST_ONLY) & (set(EXCLUDED) | set(TABLE_BY_NAME))
    assert len(TABLE_BY_NAME) == len(TABLE), "an entry point is tabled twice"
    missing = sorted(set(names) - set(TABLE_BY_NAME) - set(EXCLUDED) - set(HOST_ONLY))
    assert not missing, "neither tabled nor excluded: %s" % missing
    stale = sorted((set(TABLE_BY_NAME) | set(EXCLUDED) | set(HOST_ONLY)) - set(names))
    assert not stale, "tabled or excluded, but no int-returning entry point with a pointer: %s" % stale


def test_every_pointer_parameter_is_classified():
    """A prototype that gains a pointer fails here until someone has read what the header says about it."""
    protos = prototypes()
    for e in TABLE:
        have = [nm for nm, ptr, _ in protos[e.name] if ptr]
        said = e.pointers()
        assert len(said) == len(set(said)), "%s classifies a pointer twice: %s" % (e.name, said)
        assert sorted(have) == sorted(said), "%s: pointers %s are not classified, %s are no parameters" % (
            e.name, sorted(set(have) - set(said)), sorted(set(said) - set(have)))


def test_every_integer_parameter_is_classified():
    """... and one that gains a size, a stride or an enumeration likewise."""
    protos = prototypes()
    for e in TABLE:
        have = [nm for nm, ptr, ctype in protos[e.name] if not ptr and nm != "stream" and ctype not in ("float", "double")]
        said = e.integers()
        assert len(said) == len(set(said)), "%s classifies an integer twice: %s" % (e.name, said)
        assert sorted(have) == sorted(said), "%s: integers %s are not classified, %s are no parameters" % (
            e.name, sorted(set(have) - set(said)), sorted(set(said) - set(have)))


def test_every_optional_pointer_cites_the_header():
    prose = header_prose()
    for e in TABLE:
        cites = [c for _, c in e.opt + e.optgroup] + [c for _, _, c in e.align] + ([e.ws_optional] if e.ws_optional else [])
        for c in cites:
            assert _fold(c) in prose, "%s cites words the header does not hold: %r" % (e.name, c)


def test_the_child_saw_no_device_and_loaded_no_torch():
    r = result()
    assert r["returncode"] == 0 and r["data"] is not None, \
        "the child ended with status %s in or after [%s]\n%s" % (r["returncode"], r["last"], r["stderr"])
    assert not r["data"]["error"], r["data"]["error"]
    assert r["data"]["modules"] == [], r["data"]["modules"]
    all_rows = rows()
    n_calls = len(all_rows)
    print("\nABI contract: %d entry points tabled, %d excluded, %d rows run, %.1f s wall (%.1f s in the child)" % (
        len(TABLE) + len(HOST_ONLY), len(EXCLUDED), n_calls, r["wall"], r["data"]["seconds"]))
    assert 1000 <= n_calls <= 9000
    assert {x["entry"] for x in all_rows} == set(TABLE_BY_NAME) | set(HOST_ONLY)


def test_baselines_are_accepted():
    assert not _wrong("baseline"), "\n".join(_wrong("baseline"))


def test_a_required_pointers():
    assert not _wrong("a"), "\n".join(_wrong("a"))


def test_b_optional_pointers():
    assert not _wrong("b"), "\n".join(_wrong("b"))


def test_c_sizes_and_strides():
    assert not _wrong("c"), "\n".join(_wrong("c"))


def test_d_enumerations():
    assert not _wrong("d"), "\n".join(_wrong("d"))


def test_e_workspaces():
    assert not _wrong("e"), "\n".join(_wrong("e"))


def test_f_alignment_rules():
    assert not _wrong("f"), "\n".join(_wrong("f"))


def test_g_shape_refusals_look_at_no_pointer():
    assert rows("g")
    assert not _wrong("g"), "\n".join(_wrong("g"))


def test_h_predicates_agree_with_their_entry_points():
    assert len(rows("h")) > 500
    assert not _wrong("h"), "\n".join(_wrong("h"))


def test_x_rows_of_single_entry_points():
    assert not _wrong("x"), "\n".join(_wrong("x"))


def test_int_max_reaches_the_device_only_where_pinned():
    got = sorted("%s %s" % (x["entry"], x["row"]) for x in rows("intmax")
                 if x["rc"] == x["accept"][0] and x["accept"][1] in x["err"])
    pinned = sorted(INTMAX_ACCEPTED.split("\n")[1:-1])
    assert got == pinned, "INT_MAX newly accepted: %s; no longer accepted: %s" % (
        sorted(set(got) - set(pinned)), sorted(set(pinned) - set(got)))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        sys.exit("usage: %s --child OUT.json" % sys.argv[0])
