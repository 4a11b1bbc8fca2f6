"""The seq2seq LSTM models' data pipeline with the FoV tracks held on the device.

    replaces: mycode/utility.py:264-305 (reshape2second_stacks), :359-446 (get_data), :483-517 (get_gt_target_xyz[_oth]),
              mycode/given_others_gt_mean_var_seq2seq.py:675-695 (the test loop's slicing of those arrays) and
              mycode/data_generator_including_saliency.py:93-182 (generator_train2)

The reference builds every window of every (video, target user) as float64 (N, T, 90) and, with pick_user, the other users'
windows as (num_user-1, N, T, 90) once per target - each video's data about U * T times over - and then reduces every second
to six numbers.  Every model input but the raw encoder seconds is a row of ONE small table, the per-second mean / variance
of every track.  So a TrajectoryDataset keeps, on the device, the whole seconds of every track once (secs) and that table
(feat = ops.meanvar_xyz(secs), one launch per dataset), and on the host three ints a window.  A batch is one gather launch
(ops.window_inputs) from a list of window numbers; nothing of (N, T, U-1, 30, 3) exists anywhere.
"""
import numpy as np

from .config import cfg
from .utility import _per_video_seconds

ENC_FORMS = ("raw", "mean_var")


class TrajectoryDataset:
    """The windows utility.get_data(datadb, pick_user, num_user) returns, in its row order, as tables.

    datadb: {video: {'x','y','z': (n_user, n_frame)}}; a video of fewer than 2 * cfg.running_length whole seconds (after
    cut_head_or_tail_less_than_1sec) is skipped.  stride: cfg.data_chunk_stride.  T = cfg.running_length seconds in, T out,
    the future fut_offset = (T // stride) * stride seconds after the window's start.
    pick_user=False: videos in key order, window-major then user.  pick_user=True: videos in key order, then target user,
    then window; a target's others are the video's remaining users in order (np.delete), padded up to num_user - 1 with
    np.random.randint draws in utility._pad_others' sequence - seed np.random as for get_data - or cut to the first
    num_user - 1.  cfg.time_shift and cfg.purelly_testing are not built here: ValueError.
    device=None keeps the host tables only (no library, no GPU needed): len, tables, split."""

    def __init__(self, datadb, pick_user, num_user=34, stride=None, video_keys=None, device="cuda"):
        if cfg.time_shift or cfg.purelly_testing:
            raise ValueError("TrajectoryDataset does not build cfg.time_shift / cfg.purelly_testing windows")
        T, fps = int(cfg.running_length), int(cfg.fps)
        stride = int(cfg.data_chunk_stride if stride is None else stride)
        if not 1 <= stride <= T:
            raise ValueError("stride must be in [1, %d], got %d" % (T, stride))
        if pick_user and num_user < 2:
            raise ValueError("pick_user needs num_user >= 2")
        self.pick_user, self.num_user, self.stride = bool(pick_user), int(num_user), stride
        self.T_in = self.T_out = T
        self.fps = fps
        self.fut_offset = (T // stride) * stride
        self.n_others = self.num_user - 1 if self.pick_user else 0
        keys = list(datadb.keys()) if video_keys is None else list(video_keys)
        secs, sample, others_base = [], [], []
        row0 = 0
        for vid in keys:
            s = _per_video_seconds(datadb[vid])                      # (U, S, 3*fps)
            U, S = s.shape[:2]
            if S < 2 * T:
                continue
            W = (S - T) // stride + 1 - T // stride                  # reshape2second_stacks' window count
            starts = stride * np.arange(W)
            track = row0 + S * np.arange(U)                          # a track: S contiguous rows
            if not self.pick_user:
                blk = np.zeros((W, U, 3), np.int64)
                blk[:, :, 0] = track[None, :]
                blk[:, :, 2] = starts[:, None]
                sample.append(blk.reshape(-1, 3))
            else:
                for target in range(U):
                    oth = np.delete(np.arange(U), target)
                    n_real = len(oth)
                    if n_real < self.n_others:
                        oth = np.concatenate([oth, [oth[np.random.randint(n_real)] for _ in range(n_real, self.n_others)]])
                    blk = np.zeros((W, 3), np.int64)
                    blk[:, 0] = track[target]
                    blk[:, 1] = len(others_base)
                    blk[:, 2] = starts
                    sample.append(blk)
                    others_base.append(track[oth[:self.n_others].astype(np.int64)])
            secs.append(s.reshape(U * S, 3 * fps))
            row0 += U * S
        if row0 >= 2 ** 31:
            raise ValueError("more than 2^31 seconds of tracks")
        self._secs = np.concatenate(secs) if secs else np.zeros((0, 3 * fps))
        self._sample = (np.concatenate(sample) if sample else np.zeros((0, 3), np.int64)).astype(np.int32)
        self._others_base = np.asarray(others_base, np.int32).reshape(-1, self.n_others) if self.pick_user else None
        self.device = device
        self._dev = None
        if device is not None:
            import torch
            from . import ops
            d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            dsecs = d(self._secs.astype(np.float32))
            self._dev = {"secs": dsecs, "feat": ops.meanvar_xyz(dsecs, fps) if len(dsecs) else dsecs.new_zeros((0, 6)),
                         "sample": d(self._sample), "others_base": d(self._others_base) if self.n_others else None}

    def __len__(self):
        return len(self._sample)

    def tables(self):
        """The host arrays: secs float64 (rows, 3*fps), every track's whole seconds, a track a contiguous run of rows;
        sample int32 (N, 3) = [first row of the target's track, row of others_base, first second of the window];
        others_base int32 (pairs, num_user-1) or None; the ints T_in, T_out, fut_offset.  Window i reads the target's rows
        sample[i, 0] + sample[i, 2] + (0 .. T_in-1) and, for the future, + fut_offset + (0 .. T_out-1); slot j of its others
        others_base[sample[i, 1], j] + sample[i, 2] + fut_offset + (0 .. T_out-1)."""
        return {"secs": self._secs, "sample": self._sample, "others_base": self._others_base, "T_in": self.T_in,
                "T_out": self.T_out, "fut_offset": self.fut_offset}

    def _view(self, lo, hi):
        """Windows lo .. hi-1 as a dataset on the same tables (host and device): nothing is copied but the slice's view."""
        v = object.__new__(TrajectoryDataset)
        v.__dict__.update(self.__dict__)
        v._sample = self._sample[lo:hi]
        if self._dev is not None:
            v._dev = dict(self._dev, sample=self._dev["sample"][lo:hi])
        return v

    def split(self, fraction):
        """(the leading int(len * fraction) windows, the rest): Keras's held-out tail, as views on the same device data."""
        if not 0.0 <= fraction <= 1.0:
            raise ValueError("fraction must be in [0, 1]")
        k = int(len(self) * fraction)
        return self._view(0, k), self._view(k, len(self))

    def _gather(self, sample, names, enc):
        """ops.window_inputs of the device sample rows `sample` (n, 3), in the models' shapes."""
        from . import ops
        if self._dev is None:
            raise RuntimeError("this TrajectoryDataset was built with device=None: host tables only")
        if enc not in ENC_FORMS:
            raise ValueError("enc must be one of %r, got %r" % (ENC_FORMS, enc))
        dv = self._dev
        out = ops.window_inputs(dv["secs"], dv["feat"], sample, dv["others_base"], self.T_in, self.T_out, self.fut_offset,
                                enc_width=6 if enc == "mean_var" else 3 * self.fps, outputs=names)
        if "dec_in" in out:
            out["dec_in"] = out["dec_in"].unsqueeze(1)               # (b, 1, 6): the models' decoder seed
        return out

    def _names(self, future_raw):
        return ("enc", "dec_in", "target") + (("others",) if self.pick_user else ()) + (("future_raw",) if future_raw else ())

    def batch(self, index, enc="raw", future_raw=False):
        """The windows `index` (ints in [0, len), any order, repeats allowed; checked here, on the host) -> dict of float32
        device tensors: enc (b, T, 90) or, enc='mean_var', (b, T, 6); dec_in (b, 1, 6), the mean / variance of the
        encoder's last second; target (b, T, 6); with pick_user others (b, T, num_user-1, 6); with future_raw the raw
        future (b, T, 90), what generator_train2(phase='test') yields and save_decoded_sentences stores."""
        import torch
        index = np.asarray(index)
        if index.ndim != 1 or (index.size and index.dtype.kind not in "iu"):
            raise TypeError("index must be a one-dimensional array of integers")
        index = index.astype(np.int64)
        if index.size and (index.min() < 0 or index.max() >= len(self)):
            raise IndexError("window index outside [0, %d)" % len(self))
        if self._dev is None:
            raise RuntimeError("this TrajectoryDataset was built with device=None: host tables only")
        sample = torch.from_numpy(np.ascontiguousarray(self._sample[index])).to(self._dev["secs"].device)
        return self._gather(sample, self._names(future_raw), enc)

    def batch_range(self, lo, hi, enc="raw", future_raw=False):
        """batch(arange(lo, hi)) without the upload: the sample rows are a slice of the device table."""
        lo, hi = max(int(lo), 0), min(int(hi), len(self))
        if self._dev is None:
            raise RuntimeError("this TrajectoryDataset was built with device=None: host tables only")
        return self._gather(self._dev["sample"][lo:max(hi, lo)], self._names(future_raw), enc)


def gather_host(tables, index):
    """The windows `index` gathered with NumPy from TrajectoryDataset.tables(), as the tuple utility.get_data returns for
    them: (enc, future, future_input) float64 (b, T, 90) and, with others, the same three as (num_user-1, b, T, 90) - the
    test of the tables against the reference's arrays, and a way to read a window without a GPU."""
    secs, sample, ob = tables["secs"], tables["sample"][np.asarray(index, np.int64)].astype(np.int64), tables["others_base"]
    t_in, t_out = np.arange(tables["T_in"]), tables["fut_offset"] + np.arange(tables["T_out"])

    def three(first):                                                # first (..., b): a track's row of the window's start
        enc, fut = secs[first[..., None] + t_in], secs[first[..., None] + t_out]
        return enc, fut, np.concatenate((enc[..., -1:, :], fut[..., :-1, :]), axis=-2)

    out = three(sample[:, 0] + sample[:, 2])
    if ob is not None:
        out += three(ob[sample[:, 1]].astype(np.int64).T + sample[:, 2][None, :])
    return out
