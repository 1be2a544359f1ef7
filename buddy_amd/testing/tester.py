"""Test harness -- same surface as reference ``testing/tester.py:21-236`` (``Tester(args, network, diff_params, test_set,
device, in_training)``, ``load_checkpoint``, ``load_latest_checkpoint``, ``do_test``), plus ``batch_size`` /
rank sharding for utterance-batch data parallelism (utterance u -> rank u mod world; one gather at the end)."""
from __future__ import annotations

import copy
import os
import re
from datetime import date
from glob import glob

import numpy as np
import torch
from scipy.io import wavfile

from ..instantiate import instantiate
from ..utils.rng import factory_from_config
from .operators.reverb import RIROperator
from .operators.subband_filtering import BlindSubbandFiltering


def write_audio_file(x, sr, string, path="tmp"):
    """float32 wav writer (reference utils/log.py write_audio_file: <path>/<string>.wav)."""
    os.makedirs(path, exist_ok=True)
    p = os.path.join(path, string + ".wav")
    a = torch.as_tensor(x).detach().flatten().float().cpu().numpy()
    wavfile.write(p, sr, a.astype(np.float32))
    return p


def shared_rir_options(rr):
    """(shared_rir, shared_rir_max_chunks) of a ``real_recordings`` block; a config written before the keys existed means (False, 32)"""
    return bool(rr.get("shared_rir", False)), int(rr.get("shared_rir_max_chunks", 32))


def channel_options(rr):
    """(channels, reference_channel, (taps, delay, iterations)) of a ``real_recordings`` block; a config written before the keys existed means
    ("mean", 0, nara_wpe's defaults).  channels: mean = the channel mean, as always | reference = one channel | wpe = multichannel WPE on all
    channels (utils/wpe.py), its reference channel observed."""
    mode = str(rr.get("channels", "mean"))
    assert mode in ("mean", "reference", "wpe"), "real_recordings.channels is 'mean', 'reference' or 'wpe'"
    ref = int(rr.get("reference_channel", 0))
    assert ref >= 0, "real_recordings.reference_channel is a channel index >= 0"
    hp = rr.get("wpe", None) or {}
    return mode, ref, (int(hp.get("taps", 10)), int(hp.get("delay", 3)), int(hp.get("iterations", 3)))


def beamformer_options(rr):
    """(use, iterations, loading) of the ``beamformer`` block of a ``real_recordings`` block; a config written before the block existed means
    (False, 2, 1e-6).  use: the wMPDR beamformer after multichannel WPE (utils/wpe.py); it needs ``channels: wpe``."""
    bf = rr.get("beamformer", None) or {}
    use, iterations, loading = bool(bf.get("use", False)), int(bf.get("iterations", 2)), float(bf.get("loading", 1e-6))
    assert iterations >= 1, "real_recordings.beamformer.iterations is >= 1"
    assert 0.0 <= loading < float("inf"), "real_recordings.beamformer.loading is finite and >= 0"
    mode = str(rr.get("channels", "mean"))
    assert not use or mode == "wpe", f"real_recordings.beamformer.use needs real_recordings.channels: wpe (it is '{mode}'): the beamformer works on the WPE output of all channels"
    return use, iterations, loading


def denoise_options(rr):
    """(use, gain, floor_db) of the ``denoise`` block of a ``real_recordings`` block; a config written before the block existed means
    (False, "lsa", -15.0).  use: the noise tracker and spectral post-filter (utils/denoise.py) as the last stage of the front
    end, on whatever the channel rule hands the sampler.  gain: lsa | wiener; floor_db: the lowest gain in dB, a choice."""
    dn = rr.get("denoise", None) or {}
    use, gain, floor_db = bool(dn.get("use", False)), str(dn.get("gain", "lsa")), float(dn.get("floor_db", -15.0))
    assert gain in ("lsa", "wiener"), f"real_recordings.denoise.gain is 'lsa' or 'wiener' (it is '{gain}')"
    assert -120.0 <= floor_db <= 0.0, f"real_recordings.denoise.floor_db is a gain in dB in [-120, 0] (it is {floor_db})"
    return use, gain, floor_db


def rir_report_options(tester_cfg):
    """(use, octave centres) of the ``rir_report`` block of a tester config; a config written before the block existed means (False, the octaves)"""
    from ..utils.acoustics import OCTAVES
    rp = tester_cfg.get("rir_report", None)
    if rp is None:
        return False, OCTAVES
    c = rp.get("centres", None)
    return bool(rp.get("use", False)), OCTAVES if c is None else tuple(float(v) for v in c)


def _values_options(tester_cfg, block, all_values):
    """(use, values) of the report block ``block`` of a tester config; a config written before the block existed means (False, ``all_values``)"""
    bl = tester_cfg.get(block, None)
    if bl is None:
        return False, all_values
    v = bl.get("values", None)
    return bool(bl.get("use", False)), all_values if v is None else tuple(str(s) for s in v)


def metrics_options(tester_cfg):
    """(use, values) of the ``metrics`` block of a tester config; a config written before the block existed means (False, all four values)"""
    from ..utils.metrics import VALUES
    return _values_options(tester_cfg, "metrics", VALUES)


def align_options(tester_cfg):
    """(use, max_lag_ms) of the ``metrics.align`` block of a tester config: whether every pair is time-aligned before it is scored, and the search
    window in ms; a config written before the block existed means (False, 50.0)"""
    from ..utils.metrics import MAX_LAG_MS
    mt = tester_cfg.get("metrics", None)
    al = None if mt is None else mt.get("align", None)
    if al is None:
        return False, MAX_LAG_MS
    ms = al.get("max_lag_ms", None)
    return bool(al.get("use", False)), MAX_LAG_MS if ms is None else float(ms)


def srmr_options(tester_cfg):
    """use of the ``srmr`` block of a tester config; a config written before the block existed means False"""
    sm = tester_cfg.get("srmr", None)
    return False if sm is None else bool(sm.get("use", False))


def decay_options(tester_cfg):
    """use of the ``decay`` block of a tester config; a config written before the block existed means False"""
    dc = tester_cfg.get("decay", None)
    return False if dc is None else bool(dc.get("use", False))


def spectral_options(tester_cfg):
    """(use, values) of the ``spectral`` block of a tester config; a config written before the block existed means (False, all three values)"""
    from ..utils.spectral import VALUES
    return _values_options(tester_cfg, "spectral", VALUES)


def sdr_options(tester_cfg):
    """(use, taps) of the ``sdr`` block of a tester config; a config written before the block existed means (False, the four default filter lengths)"""
    from ..utils.sdr import TAPS
    sd = tester_cfg.get("sdr", None)
    if sd is None:
        return False, TAPS
    t = sd.get("taps", None)
    return bool(sd.get("use", False)), TAPS if t is None else tuple(int(m) for m in t)


class Tester:
    def __init__(self, args, network, diff_params, test_set=None, device=None, in_training=False, batch_size=1, rank=0, world_size=1):
        self.args = args
        self.network = network
        self.diff_params = copy.copy(diff_params)
        self.device = device
        self.test_set = test_set
        self.in_training = in_training
        self.batch_size, self.rank, self.world_size = batch_size, rank, world_size
        self.sampler = instantiate(args.tester.sampler, self.network, self.diff_params, self.args)
        self.paths = {}
        self.results = []
        # a batch of >= 2 * sub_batches utterances is sampled as that many concurrent sub-batches on their own HIP streams
        # (testing/concurrent.py; better occupancy); 1 = one batch, one stream.  Default ("auto", tester.sub_batches absent): 2 whenever
        # a group has >= 4 utterances -- the measured optimum (+4-5 %; 4 loses: profiles/r05_sub_batch_sweep.txt).  Results equal the single-batch run
        # row for row only with per-utterance noise streams (tester.noise.generator = philox, or a noise_factory); with the torch RNG the draw ORDER differs between the two
        # modes, so tester.sub_batches=1 is the way to reproduce a same-seed run of an earlier round.  The second sub-batch's network is a
        # replica: it shares the prepared weights and costs only its activation arena
        sb = args.tester.get("sub_batches", None) if hasattr(args.tester, "get") else None
        self.sub_batches = None if sb in (None, "auto") else int(sb)
        self._concurrent = None
        # seeded sampling (tester.noise.generator = philox, tester.noise.seed; utils/rng.py): every utterance draws from the Philox stream of
        # (seed, its name), on the GPU -- rows independent of batch, sub-batch policy, file order and world size for every user, not only under an
        # injected factory.  Default (torch, or no such block): no attribute, the torch generators in the reference's draw order.  A
        # ``noise_factory`` assigned from outside replaces this one
        factory = factory_from_config(args.tester, device)
        if factory is not None:
            self.noise_factory = factory

    # ---- checkpoints (reference :34-67): the EMA weights are what gets loaded -------------------------------------
    def load_checkpoint(self, path):
        """reference :60-67: ``it`` if present, then utils/training_utils.load_state_dict(state_dict, ema=self.network)
        (strict EMA, EMA with strict=False, shape-matched EMA, 'state_dict' key) -- never the raw 'network' weights."""
        from ..utils.training_utils import load_state_dict
        state_dict = torch.load(path, map_location="cpu", weights_only=False)
        try:
            self.it = state_dict["it"]
        except Exception:
            self.it = 0
        print("loading checkpoint")
        self._concurrent = None      # cached sub-batch replicas pin the OLD weight store: rebuild them on the reloaded parent
        return load_state_dict(state_dict, ema=self.network)

    def load_latest_checkpoint(self):
        """reference :34-58: newest ``<model_dir>/<exp_name>-<it>.pt``; strict 'ema', else 'model' with strict=False."""
        self._concurrent = None      # see load_checkpoint
        try:
            name = f"{self.args.model_dir}/{self.args.exp.exp_name}-*.pt"
            rx = re.compile(f"{self.args.exp.exp_name}-(\\d*)\\.pt")
            ids = [int(rx.search(w).groups()[0]) for w in glob(name)]
            cid = max(ids)
            state_dict = torch.load(f"{self.args.model_dir}/{self.args.exp.exp_name}-{cid}.pt", map_location="cpu", weights_only=False)
            try:
                self.network.load_state_dict(state_dict["ema"])
            except Exception as e:
                print(e)
                print("Failed to load in strict mode, trying again without strict mode")
                self.network.load_state_dict(state_dict["model"], strict=False)
            print(f"Loaded checkpoint {cid}")
            return True
        except (FileNotFoundError, ValueError):
            raise ValueError("No checkpoint found")

    # ---- unconditional ---------------------------------------------------------------------------------------------
    def sample_unconditional(self, mode):
        unc = self.args.tester.unconditional
        audio_len = self.args.exp.audio_len if "audio_len" not in unc.keys() else unc.audio_len
        if getattr(self, "noise_factory", None) is not None:
            self.sampler.noise = self.noise_factory([f"unconditional_{i}" for i in range(unc.num_samples)])
        preds = self.sampler.predict_unconditional([unc.num_samples, audio_len], self.device)
        if not self.in_training:
            for i in range(len(preds)):
                write_audio_file(preds[i], self.args.exp.sample_rate, f"unconditional_{i}", path=self.paths["unconditional"])
        return preds

    # ---- dereverberation (reference :123-163) ----------------------------------------------------------------------
    def prepare_batch(self, items, blind, noise=None):
        """clean/RIR pairs -> (seg, y, operator) for one batch of equal-length utterances."""
        sf = self.args.tester.posterior_sampling.warm_initialization.scaling_factor
        op_hp = self.args.tester.informed_dereverberation.op_hp
        segs, rirs = [], []
        for original, rir, _ in items:
            seg = torch.from_numpy(np.asarray(original)).float().to(self.device)
            segs.append(sf * seg / seg.std())       # normalised with the warm-init scaling factor (reference :135, appendix B.13)
            rirs.append(torch.as_tensor(np.asarray(rir), dtype=torch.float32))
        seg = torch.stack(segs)
        with torch.no_grad():
            operator_ref = RIROperator(op_hp, time_kernel_size=max(r.shape[-1] for r in rirs), sample_rate=self.args.exp.sample_rate, device=self.device)
            operator_ref.update_params(rirs if len(rirs) > 1 else rirs[0])
            y = operator_ref.degradation(seg)
            operator = operator_ref
            if blind:
                operator = self._blind_operator(len(items), seg.shape[-1], noise)
        return seg, y, operator, rirs

    def _blind_operator(self, n, length, noise, groups=None):
        """a fresh blind operator for ``n`` utterances of ``length`` samples: own parameters / RIR estimate per row, or per group of rows (``groups``)"""
        assert self.args.tester.blind_dereverberation.operator == "subband_filtering"
        operator = BlindSubbandFiltering(self.args.tester.informed_dereverberation.op_hp, sample_rate=self.args.exp.sample_rate, num_utts=n, noise=noise,
                                         device=self.device, length=length, groups=groups)
        operator.update_H(use_noise=True)
        return operator

    def _num_sub_batches(self, n):
        """how many concurrent sub-batches a group of ``n`` utterances is sampled as (1 = one batch, one stream)"""
        S = self.sub_batches if self.sub_batches is not None else (2 if n >= 4 else 1)
        return S if S > 1 and n >= 2 * S and str(self.device).startswith("cuda") else 1

    def test_dereverberation(self, mode, blind=False):
        if self.test_set is None or len(self.test_set) == 0:
            print("No test set specified / no samples found")
            return
        mine = [i for i in range(len(self.test_set)) if i % self.world_size == self.rank]
        sr = self.args.exp.sample_rate
        local = {}
        report = blind and rir_report_options(self.args.tester)[0] and not self.in_training and bool(self.paths)
        rep = []         # room-acoustics report: (name, estimated RIR, true RIR, the operator's parameters of that row) per written RIR wav
        scoring = metrics_options(self.args.tester)[0] and not self.in_training and bool(self.paths)
        scored = []      # evaluation, spectral and SDR reports: (name, clean, degraded, reconstructed) per written utterance, as written to the wavs
        spectral_on = spectral_options(self.args.tester)[0] and not self.in_training and bool(self.paths)
        sdr_on = sdr_options(self.args.tester)[0] and not self.in_training and bool(self.paths)
        decay_on = decay_options(self.args.tester) and not self.in_training and bool(self.paths)
        srmr_on = srmr_options(self.args.tester) and not self.in_training and bool(self.paths)
        heard = []     # SRMR and decay-time reports: (name, degraded, reconstructed, clean) per written utterance, each row with the rate of its wav
        for s in range(0, len(mine), self.batch_size):
            idx = mine[s:s + self.batch_size]
            items = [self.test_set[i] + (i,) for i in idx]
            groups = {}
            for it in items:                      # only equal-length utterances share a batch
                groups.setdefault(len(it[0]), []).append(it)
            for L, grp in groups.items():
                uidx = [it[3] for it in grp]
                grp = [it[:3] for it in grp]
                # parity runs: one injected noise stream per utterance, shared by the sampler AND the blind operator (random phases,
                # update_H(use_noise=True), per-step RIR-regulariser draws) in the reference's call order; otherwise the torch RNG
                self.sampler.noise = self.noise_factory([it[2] for it in grp]) if getattr(self, "noise_factory", None) is not None else None
                S = self._num_sub_batches(len(grp))
                if S > 1:
                    seg, y, pred, est, rirs = self._sample_concurrent(grp, L, blind, S)
                else:
                    seg, y, operator, rirs = self.prepare_batch(grp, blind, noise=self.sampler.noise)
                    pred = self.sampler.predict_conditional(y, operator, shape=(len(grp), L), blind=blind)
                    est = self.sampler.operator.get_time_RIR().detach().cpu() if blind else None
                par = self._operator_parameters(S) if report else None
                for b, (_, _, filename) in enumerate(grp):
                    name = os.path.basename(filename)[:-4]
                    self.results.append((name, pred[b].detach().cpu()))
                    local[uidx[b]] = pred[b].detach()
                    if self.in_training or not self.paths:
                        continue
                    write_audio_file(seg[b], sr, name, path=self.paths[mode + "original"])
                    write_audio_file(y[b], sr, name, path=self.paths[mode + "degraded"])
                    p = write_audio_file(pred[b], sr, name, path=self.paths[mode + "reconstructed"])
                    write_audio_file(rirs[b], sr, name, path=self.paths[mode + "true_rir"])
                    if blind:
                        write_audio_file(est[b] if est.dim() == 2 else est, sr, name, path=self.paths[mode + "estimated_rir"])
                    if report:
                        rep.append((name, est[b] if est.dim() == 2 else est, rirs[b], {k: v if k == "freqs" else v[b] for k, v in par.items()}))
                    if scoring or spectral_on or sdr_on:
                        scored.append((name, seg[b].detach(), y[b].detach(), pred[b].detach()))
                    if srmr_on or decay_on:
                        heard.append((name, (y[b].detach(), sr), (pred[b].detach(), sr), (seg[b].detach(), sr)))
                    print(p)
        if report:
            self._write_rir_report(mode, rep, sr)
        if scoring:
            self._write_metrics_report(mode, scored, sr)
        if spectral_on:
            self._write_spectral_report(mode, scored, sr)
        if sdr_on:
            self._write_sdr_report(mode, scored, sr)
        if srmr_on:
            self._write_srmr_report(mode, heard)
        if decay_on:
            self._write_decay_report(mode, heard)
        # utterance-batch data parallelism: ONE gather at the end of the run (RCCL over xGMI on the GPU box) -- afterwards every rank, in
        # particular rank 0, holds all predictions in utterance order, independent of the world size
        from .. import dist as bdist
        rows = bdist.gather_ragged([local[i] for i in mine], len(self.test_set), self.rank, self.world_size, device=self.device)
        self.gathered = [(os.path.basename(self.test_set[i][2])[:-4], rows[i].detach().cpu()) for i in range(len(self.test_set))]

    def _operator_parameters(self, S):
        """``acoustic_parameters()`` of the operators the last group was sampled with, rows in order (``S`` > 1: one operator per sub-batch)"""
        ops = [sb.s.operator for sb in self._concurrent.last] if S > 1 else [self.sampler.operator]
        pars = [op.acoustic_parameters() for op in ops]
        return {"freqs": pars[0]["freqs"], "T60": torch.cat([p["T60"] for p in pars]), "weights": torch.cat([p["weights"] for p in pars])}

    def _write_rir_report(self, mode, rep, sr):
        """Room-acoustics report of a blind mode (``tester.rir_report.use``; utils/acoustics.py), once per mode after sampling: ``acoustics.csv`` (the
        six ISO 3382-1 values per written RIR wav and band; with true RIRs also theirs and the errors of the estimate) and ``parameters.csv`` (the
        fitted T60 and weight per knot) next to the RIR wavs.  ``rep``: (wav name, estimated RIR, true RIR or None, parameters of that operator
        row).  Every rank writes its own rows (``acoustics.rank<r>.csv`` when there are several); nothing is gathered."""
        from ..utils import acoustics
        self.rir_report = None
        if not rep:
            return
        centres = rir_report_options(self.args.tester)[1]
        names = [r[0] for r in rep]
        est = acoustics.rir_acoustics(torch.stack([r[1].float() for r in rep]).to(self.device), int(sr), centres=centres)
        true = None
        if rep[0][2] is not None:          # true RIRs of different lengths: one zero-padded batch, analysed up to each row's own length
            lens = [int(r[2].numel()) for r in rep]
            rows = torch.zeros(len(rep), max(lens), dtype=torch.float32)
            for b, r in enumerate(rep):
                rows[b, :lens[b]] = r[2].flatten()
            true = acoustics.rir_acoustics(rows.to(self.device), int(sr), lens=lens, centres=centres)
        params = {"freqs": rep[0][3]["freqs"], "T60": torch.stack([r[3]["T60"] for r in rep]), "weights": torch.stack([r[3]["weights"] for r in rep])}
        tag = f".rank{self.rank}" if self.world_size > 1 else ""
        base = self.paths[mode + "estimated_rir"]
        acoustics.write_report(os.path.join(base, f"acoustics{tag}.csv"), acoustics.report_rows(names, est, true))
        acoustics.write_parameters(os.path.join(base, f"parameters{tag}.csv"), acoustics.parameter_rows(names, params))
        self.rir_report = dict(names=names, estimated=est, true=true, parameters=params)

    def _write_metrics_report(self, mode, scored, sr):
        """Evaluation report of a paired mode (``tester.metrics.use``; utils/metrics.py), once per mode after sampling: ``metrics.csv`` (per written
        utterance SI-SDR, STOI, ESTOI and LSD of the degraded and of the reconstructed signal against the clean one, and the difference) and
        ``metrics_summary.csv`` (n, mean, median, std per column) in the mode's directory.  ``scored``: (wav name, clean, degraded, reconstructed),
        the float32 rows the wavs hold; equal lengths are scored as one batch.  ``tester.metrics.align.use``: the degraded and the reconstructed signal
        are each shifted by their own integer lag against the clean one and trimmed to the overlap first (``metrics.align``), and the lags, their
        correlations and flags are further columns.  Every rank writes its own rows (``metrics.rank<r>.csv`` when there are
        several); nothing is gathered -- ``tools/evaluate.py`` scores the directory of a multi-rank run as a whole."""
        from ..utils import metrics
        self.metrics_report = self._write_pair_report(mode, scored, sr, metrics, "metrics", metrics_options(self.args.tester)[1])

    def _write_pair_report(self, mode, scored, sr, module, stem, values):
        """the body of the paired reports: ``module`` (utils/metrics.py, utils/spectral.py or utils/sdr.py) scores the degraded and the reconstructed rows of
        ``scored`` against the clean ones, equal lengths as one batch, after ``tester.metrics.align`` where it is in use, and writes ``<stem>.csv`` and
        ``<stem>_summary.csv`` into the mode's directory -> the rows, or None where nothing was scored"""
        if not scored:
            return None
        use_align, max_lag_ms = align_options(self.args.tester)
        window = max_lag_ms if use_align else None
        groups = {}
        for i, r in enumerate(scored):
            groups.setdefault(int(r[1].numel()), []).append(i)
        rows = [None] * len(scored)
        for idx in groups.values():
            clean, deg, rec = (torch.stack([scored[i][k].flatten().float() for i in idx]).to(self.device) for k in (1, 2, 3))
            inp = module.evaluate(deg, clean, int(sr), values=values, align=window)
            out = module.evaluate(rec, clean, int(sr), values=values, align=window)
            for i, row in zip(idx, module.report_rows([scored[i][0] for i in idx], inp, out)):
                rows[i] = row
        tag = f".rank{self.rank}" if self.world_size > 1 else ""
        module.write_report(os.path.join(self.paths[mode], f"{stem}{tag}.csv"), rows)
        module.write_report(os.path.join(self.paths[mode], f"{stem}_summary{tag}.csv"), module.summary_rows(rows))
        return rows

    def _write_spectral_report(self, mode, scored, sr):
        """Spectral distortion report of a paired mode (``tester.spectral.use``; utils/spectral.py), once per mode after sampling:
        ``spectral.csv`` (per written utterance the cepstral distance, LLR and fwSegSNR of the degraded and of the reconstructed signal against the clean
        one, and the difference) and ``spectral_summary.csv`` (n, mean, median, std per column) in the mode's directory.  ``scored`` as in
        ``_write_metrics_report``, and ``tester.metrics.align`` is honoured in the same way, so both reports score the same trimmed pairs.  Every rank
        writes its own rows (``spectral.rank<r>.csv`` when there are several); nothing is gathered -- ``tools/spectral.py`` scores the directory of a
        multi-rank run as a whole."""
        from ..utils import spectral
        self.spectral_report = self._write_pair_report(mode, scored, sr, spectral, "spectral", spectral_options(self.args.tester)[1])

    def _write_sdr_report(self, mode, scored, sr):
        """Projection SDR report of a paired mode (``tester.sdr.use``; utils/sdr.py), once per mode after sampling: ``sdr.csv`` (per
        written utterance the BSS-Eval SDR of the degraded and of the reconstructed signal against the clean one at every filter length of
        ``tester.sdr.taps``, and the difference) and ``sdr_summary.csv`` (n, mean, median, std per column) in the mode's directory.  ``scored`` as in
        ``_write_metrics_report``, and ``tester.metrics.align`` is honoured in the same way.  Every rank writes its own rows (``sdr.rank<r>.csv`` when
        there are several); nothing is gathered -- ``tools/sdr.py`` scores the directory of a multi-rank run as a whole."""
        from ..utils import sdr
        self.sdr_report = self._write_pair_report(mode, scored, sr, sdr, "sdr", sdr_options(self.args.tester)[1])

    def _write_srmr_report(self, mode, items):
        """SRMR report of a mode (``tester.srmr.use``; utils/srmr.py), once per mode after sampling: ``srmr.csv`` (per written
        utterance the score of the degraded and of the reconstructed signal, their difference, and in a paired mode the clean signal's) and
        ``srmr_summary.csv`` (n, mean, median, std per score column) in the mode's directory.  ``items``: (wav name, degraded, reconstructed, clean or
        None), each a (row, rate) pair: the float32 samples its wav holds at the rate the wav is written at.  Every rank writes its own rows
        (``srmr.rank<r>.csv`` when there are several); nothing is gathered -- ``tools/srmr.py`` scores the directory of a multi-rank run as a whole."""
        from ..utils import srmr
        self.srmr_report = None
        if not items:
            return
        paired = items[0][3] is not None
        cols = [srmr.score_signals([(it[k][0].flatten().float(), it[k][1]) for it in items], self.device) for k in ((1, 2, 3) if paired else (1, 2))]
        rows = srmr.report_rows([it[0] for it in items], cols[0], cols[1], cols[2] if paired else None)
        tag = f".rank{self.rank}" if self.world_size > 1 else ""
        srmr.write_report(os.path.join(self.paths[mode], f"srmr{tag}.csv"), rows)
        srmr.write_report(os.path.join(self.paths[mode], f"srmr_summary{tag}.csv"), srmr.summary_rows(rows))
        self.srmr_report = rows

    def _write_decay_report(self, mode, items):
        """Decay-time report of a mode (``tester.decay.use``; utils/decay.py), once per mode after sampling: ``decay.csv`` (per
        written utterance the blind decay time of the degraded and of the reconstructed signal, broadband and per octave band, their difference, the
        kept regions, the spread and the flags, and in a paired mode the clean signal's, the floor speech itself sets) and ``decay_summary.csv`` (n,
        mean, median, std per decay-time column) in the mode's directory.  ``items`` as in ``_write_srmr_report``; rank-tagged names as there."""
        from ..utils import decay
        self.decay_report = None
        if not items:
            return
        paired = items[0][3] is not None
        cols = [decay.score_signals([(it[k][0].flatten().float(), it[k][1]) for it in items], self.device) for k in ((1, 2, 3) if paired else (1, 2))]
        rows = decay.report_rows([it[0] for it in items], cols[0], cols[1], cols[2] if paired else None)
        tag = f".rank{self.rank}" if self.world_size > 1 else ""
        decay.write_report(os.path.join(self.paths[mode], f"decay{tag}.csv"), rows)
        decay.write_report(os.path.join(self.paths[mode], f"decay_summary{tag}.csv"), decay.summary_rows(rows))
        self.decay_report = rows

    def _sample_concurrent(self, grp, L, blind, S):
        """one equal-length group as ``S`` concurrent sub-batches (testing/concurrent.py)"""
        from .concurrent import split_rows
        self._concurrent_for(S)
        parts = split_rows(len(grp), S)
        noise = self.sampler.noise
        segs, ys, ops, rirs, noises = [], [], [], [], []
        for lo, hi in parts:
            nz = None if noise is None else noise[lo:hi]
            seg, y, op, rr = self.prepare_batch(grp[lo:hi], blind, noise=nz)
            segs.append(seg); ys.append(y); ops.append(op); rirs += rr; noises.append(nz)
        pred, est = self._predict_concurrent(ys, ops, blind, None if noise is None else noises, S)
        return torch.cat(segs), torch.cat(ys), pred, est, rirs

    def _concurrent_for(self, S):
        from .concurrent import ConcurrentSampler
        if self._concurrent is None or self._concurrent_S != S:
            self._concurrent, self._concurrent_S = ConcurrentSampler(self.args, self.network, self.diff_params, S), S
        return self._concurrent

    def _predict_concurrent(self, ys, ops, blind, noises, S):
        """``S`` prepared sub-batches (observations, operators, noise streams) -> (estimates, estimated RIRs or None), rows in order"""
        preds = self._concurrent_for(S).predict_conditional(ys, ops, blind, noises)
        est = None
        if blind:
            e = [sb.s.operator.get_time_RIR().detach().cpu() for sb in self._concurrent.last]
            est = torch.cat([v if v.dim() == 2 else v[None] for v in e])
        return torch.cat(preds), est

    def sample_observed(self, y, names, groups=None):
        """Blind dereverberation of GIVEN observations: ``y`` (n, L), each row an independent utterance with its own operator row and, with a
        ``noise_factory``, its own noise stream called ``names[b]``.  The sampling half of ``test_dereverberation`` (same sub-batch policy) without
        the clean/RIR synthesis.  ``groups`` (n ints, contiguous, from 0): rows of one group share one operator row set, i.e. one RIR estimate;
        sub-batches then never split a group.  Returns (estimates (n, L), estimated RIRs (n, M) on the CPU)."""
        from .concurrent import split_groups, split_rows
        n, L = y.shape
        noise = self.noise_factory(list(names)) if getattr(self, "noise_factory", None) is not None else None
        self.sampler.noise = noise
        S = self._num_sub_batches(n)
        parts = split_rows(n, S) if groups is None else split_groups(groups, S)
        with torch.no_grad():
            if len(parts) > 1:
                S = len(parts)
                noises = None if noise is None else [noise[lo:hi] for lo, hi in parts]
                ops = [self._blind_operator(hi - lo, L, None if noise is None else noise[lo:hi],
                                            None if groups is None else [g - groups[lo] for g in groups[lo:hi]]) for lo, hi in parts]
                self._sampled_concurrently = True
                return self._predict_concurrent([y[lo:hi].contiguous() for lo, hi in parts], ops, True, noises, S)
            operator = self._blind_operator(n, L, noise, groups)
        self._sampled_concurrently = False
        pred = self.sampler.predict_conditional(y.contiguous(), operator, shape=(n, L), blind=True)
        est = self.sampler.operator.get_time_RIR().detach().cpu()
        return pred, est if est.dim() == 2 else est[None]

    # ---- real recordings: any rate, any length, no clean signal or true RIR (no reference counterpart) -----------------------------------------
    def test_real_recordings(self, mode):
        """Every file of an ``AudioFolder`` -> its dereverberated version.  Per file, on the GPU: resample to the model's rate, scale to
        ``gain * scaling_factor / std`` (``real_recordings.level: active``: by the active speech level instead, ``utils/level.py``, with one line per
        file in ``levels.csv``); files of at least one chunk are cut into equal overlapping chunks (testing/longform.py) and the chunks of
        ALL files are sampled as one pool of independent utterances in batches of ``batch_size``; then level match, cross-fade, undo the scaling,
        resample back.  Files go to ranks by index; every rank writes its own, nothing is gathered.  ``real_recordings.shared_rir``: the chunks
        of a file are tied rows of one operator -- one RIR estimate per file, fitted to all its chunks; a batch then never splits a file
        (``longform.pool_plan_shared``).  ``self.rirs[name]`` keeps the per-chunk RIR estimates in both modes.  ``real_recordings.denoise.use``:
        the spectral post-filter (utils/denoise.py) follows the channel rule, once per file before the scaling; ``denoised/`` holds what the sampler
        observed, ``denoise.csv`` one line per file, and ``degraded/`` and ``wpe/`` the bytes of the run without it."""
        from . import longform
        from ..utils.resample import resample
        if self.test_set is None or len(self.test_set) == 0:
            print("No test set specified / no samples found")
            return
        rr = self.args.tester.real_recordings
        ps = self.args.tester.posterior_sampling
        sr = int(self.args.exp.sample_rate)
        from ..utils import level as lv
        level_rule, ref_activity = lv.level_options(rr)      # level=active without a reference activity stops here, before anything is sampled
        chunk = int(self.args.exp.audio_len) if rr.get("chunk_seconds", None) is None else int(round(float(rr.chunk_seconds) * sr))
        overlap = int(round(float(rr.get("overlap_seconds", 0.5)) * sr))
        out_rate = str(rr.get("output_rate", "input"))
        assert out_rate in ("input", "model"), "real_recordings.output_rate is 'input' or 'model'"
        to_input_rate = out_rate == "input"
        csm = ps.get("constraint_speech_magnitude", None)
        level = bool(csm is not None and csm.get("use", False))      # the condition of dereverberate_long
        self.skipped = []
        files = []
        levels = []    # level=active: one line of levels.csv per file
        ch_mode, ref_ch, wpe_hp = channel_options(rr)
        bf_use, bf_iterations, bf_loading = beamformer_options(rr)      # use: true without channels: wpe stops here, before anything is sampled
        dn_use, dn_gain, dn_floor = denoise_options(rr)
        dn_rows = []   # denoise.use: one line of denoise.csv per file
        if dn_use:
            from ..utils import denoise as dnz

        def plain_gain(sig):
            """denoise.use: the gain the run WITHOUT the post-filter gives the file, from the signal in front of it -- ``degraded/`` and ``wpe/`` are
            written with it, so they hold the bytes of that run"""
            g = float(rr.get("gain", 1.0)) * float(ps.warm_initialization.scaling_factor) / float(sig.std())
            if level_rule == "active":
                m = lv.speech_level(sig[None], sr)
                if int(m.flags[0]) == 0:
                    g = lv.active_gain(rr.get("gain", 1.0), ps.warm_initialization.scaling_factor, float(m.active_rms[0]), ref_activity)
            return g

        for i in range(self.rank, len(self.test_set), self.world_size):
            recorded = None      # channels != mean: the reference channel as recorded, at the model's rate (y is then what the sampler observes)
            if ch_mode == "mean":
                audio, fs, filename = self.test_set[i]
                y = resample(torch.from_numpy(np.asarray(audio)).float().to(self.device), fs, sr)
            else:
                y, recorded, audio, fs, filename = self._observed_channel(i, ch_mode, ref_ch, wpe_hp, sr, (bf_iterations, bf_loading) if bf_use else None)
                if y is None:
                    self.skipped.append(filename)
                    continue
            front = None         # denoise.use: the signal in front of the post-filter
            if dn_use:           # the last stage of the front end: once per file, on the whole signal the sampler would observe, before the level scaling
                front = y
                dn_res = dnz.denoise(y[None].contiguous(), gain=dn_gain, floor_db=dn_floor)
                y = dn_res.out[0]
            std = float(y.std()) if y.numel() > 1 else 0.0
            if y.numel() < 1024 or not std > 0.0:       # below what the HIP STFT / loss kernels take (operators/reverb.py), or digital silence
                print(f"skipping {filename}: {y.numel()} samples at {sr} Hz" + ("" if y.numel() < 1024 else ", silent"))
                self.skipped.append(filename)
                continue
            g = float(rr.get("gain", 1.0)) * float(ps.warm_initialization.scaling_factor) / std
            if level_rule == "active":      # scale by the level while speech is active (utils/level.py), not by a std that falls with every pause
                m = lv.speech_level(y[None], sr)
                rule = "active"
                if int(m.flags[0]) != 0:
                    rule = "std"
                    print(f"{filename}: the active level is flagged {lv.flag_text(m.flags[0])}: scaled by its std instead")
                else:
                    g = lv.active_gain(rr.get("gain", 1.0), ps.warm_initialization.scaling_factor, float(m.active_rms[0]), ref_activity)
                levels += lv.report_rows([os.path.basename(filename)[:-4]], m, [{"rule": rule, "g": g}])
            files.append(dict(name=os.path.basename(filename)[:-4], fs=int(fs), n_in=len(audio), y=g * y, g=g))
            g_plain = g
            if dn_use:
                dn_rows += dnz.report_rows([files[-1]["name"]], dn_res)
                g_plain = plain_gain(front)
                files[-1]["front"] = g_plain * front
            if recorded is not None:
                files[-1]["recorded"] = g_plain * recorded
        shared, max_rows = shared_rir_options(rr)
        lengths = [f["y"].numel() for f in files]
        if shared:
            cuts, batches = longform.pool_plan_shared(lengths, chunk, overlap, self.batch_size, max_rows)
            for f, (starts, _) in zip(files, cuts):
                f["runs"] = longform.run_bounds(len(starts), max_rows)
                if len(f["runs"]) > 1:
                    print(f"{f['name']}: {len(starts)} chunks, more than shared_rir_max_chunks={max_rows}: {len(f['runs'])} runs with one RIR estimate each")
        else:
            cuts, batches = longform.pool_plan(lengths, chunk, overlap, self.batch_size)
        for f, (starts, clen) in zip(files, cuts):
            f["parts"] = torch.stack([f["y"][s:s + clen] for s in starts])
            f["est"], f["rir"], f["par"] = [None] * len(starts), [None] * len(starts), [None] * len(starts)
        writing = not self.in_training and bool(self.paths)
        self.levels = levels if level_rule == "active" else None
        if writing and level_rule == "active":
            lv.write_report(os.path.join(self.paths[mode], "levels.csv" if self.world_size == 1 else f"levels.rank{self.rank}.csv"), levels)
        self.denoise_rows = dn_rows if dn_use else None
        if writing and dn_use:
            dnz.write_report(os.path.join(self.paths[mode], "denoise.csv" if self.world_size == 1 else f"denoise.rank{self.rank}.csv"), dn_rows)
        report = writing and rir_report_options(self.args.tester)[0]
        srmr_on = writing and srmr_options(self.args.tester)
        decay_on = writing and decay_options(self.args.tester)
        heard = []     # SRMR and decay-time reports: (name, degraded at the model's rate, reconstructed at its own rate, no clean signal) per written file
        for batch in batches:
            yb = torch.stack([files[f]["parts"][k] for f, k in batch])
            pred, est = self.sample_observed(yb, [f"{files[f]['name']}_c{k}.wav" for f, k in batch],
                                             groups=longform.shared_groups(cuts, batch, max_rows) if shared else None)
            for b, (f, k) in enumerate(batch):
                files[f]["est"][k], files[f]["rir"][k] = pred[b].detach(), est[b]
            if report:
                par = self._operator_parameters(len(self._concurrent.last) if self._sampled_concurrently else 1)
                for b, (f, k) in enumerate(batch):
                    files[f]["par"][k] = {key: v if key == "freqs" else v[b] for key, v in par.items()}
        rep = []
        self.rirs = {f["name"]: list(f["rir"]) for f in files}
        for f, (starts, _) in zip(files, cuts):
            est = torch.stack(f["est"])
            if level and len(starts) > 1:
                est = est * longform.chunk_gains(f["parts"], f["y"]).to(est.dtype)
            pred = longform.merge(est, starts, f["y"].numel()) / f["g"]
            if to_input_rate:
                pred = resample(pred.contiguous(), sr, f["fs"])[:f["n_in"]]
            self.results.append((f["name"], pred.detach().cpu()))
            if not writing:
                continue
            front = f.get("front", f["y"])            # denoise.use: the front end's output before the post-filter, with the gain of the run without it
            degraded = f.get("recorded", front)       # channels != mean: the reference channel as recorded, with the file's gain
            write_audio_file(degraded, sr, f["name"], path=self.paths[mode + "degraded"])
            if ch_mode == "wpe":                      # the array front end's output: what the sampler observed, unless the post-filter follows
                write_audio_file(front, sr, f["name"], path=self.paths[mode + "wpe"])
            if dn_use:                                # what the sampler observed
                write_audio_file(f["y"], sr, f["name"], path=self.paths[mode + "denoised"])
            p = write_audio_file(pred, f["fs"] if to_input_rate else sr, f["name"], path=self.paths[mode + "reconstructed"])
            if srmr_on or decay_on:
                heard.append((f["name"], (degraded.detach(), sr), (pred.detach(), f["fs"] if to_input_rate else sr), None))
            if shared:       # one estimate per file (per run where shared_rir_max_chunks cut it): the chunks of a run hold the same RIR
                for j, (lo, _) in enumerate(f["runs"]):
                    write_audio_file(f["rir"][lo], sr, f["name"] if len(f["runs"]) == 1 else f"{f['name']}_r{j}", path=self.paths[mode + "estimated_rir"])
                    rep.append((f["name"] if len(f["runs"]) == 1 else f"{f['name']}_r{j}", f["rir"][lo], None, f["par"][lo]))
            else:
                for k, r in enumerate(f["rir"]):
                    write_audio_file(r, sr, f"{f['name']}_c{k}", path=self.paths[mode + "estimated_rir"])
                    rep.append((f"{f['name']}_c{k}", r, None, f["par"][k]))
            print(p)
        if report:
            self._write_rir_report(mode, rep, sr)
        if srmr_on:
            self._write_srmr_report(mode, heard)
        if decay_on:
            self._write_decay_report(mode, heard)

    def _observed_channel(self, i, ch_mode, ref_ch, wpe_hp, sr, bf_hp=None):
        """file ``i`` read with its channels unmixed (``real_recordings.channels: reference | wpe``) -> (observed signal, reference channel as
        recorded, the reference channel at the file's rate, fs, filename), the first two at the model's rate on the GPU; the observed signal is
        None for a file to skip.  wpe: ALL channels through one ``wpe_mc_dereverb`` call (B = 1, the whole file), the reference channel of the
        result observed; a mono file is D = 1 through the same entry.  A file the entry cannot take is skipped; a file with fewer frames than
        D * taps + delay (R rank-deficient) is processed as ``reference``.  ``bf_hp`` = (iterations, loading): the wMPDR beamformer towards the
        reference channel follows the WPE in the same library call (``wpe_mc_mpdr_dereverb``) and its one output is what is observed."""
        from ..utils import wpe as W
        from ..utils.resample import resample
        chans, fs, filename = self.test_set.channels(i)
        C = chans.shape[0]
        if ref_ch >= C:
            print(f"skipping {filename}: {C} channel(s), reference_channel is {ref_ch}")
            return None, None, None, fs, filename
        taps, delay, iterations = wpe_hp
        if ch_mode == "wpe" and not W.supported(C, taps):
            print(f"skipping {filename}: {C} channels x {taps} taps is outside what the WPE kernel takes (at most {W.MAX_CHANNELS} channels, "
                  f"channels x taps <= {W.MAX_FILTER})")
            return None, None, None, fs, filename
        if ch_mode == "reference":
            y = resample(torch.from_numpy(chans[ref_ch]).float().to(self.device), fs, sr)
            return y, y, chans[ref_ch], fs, filename
        ya = resample(torch.from_numpy(chans).float().to(self.device), fs, sr)                     # (C, n) at the model's rate
        recorded = ya[ref_ch]
        if W.frames(ya.shape[1]) < C * taps + delay:
            print(f"{filename}: {W.frames(ya.shape[1])} frames, fewer than channels x taps + delay = {C * taps + delay}: processed as its reference channel, without WPE")
            return recorded, recorded, chans[ref_ch], fs, filename
        if bf_hp is not None:
            y = W.wpe_mc_mpdr_dereverb(ya[None].contiguous(), taps=taps, delay=delay, iterations=iterations, reference=ref_ch, bf_iterations=bf_hp[0],
                                       loading=bf_hp[1])[0]
            return y, recorded, chans[ref_ch], fs, filename
        y = W.wpe_mc_dereverb(ya[None].contiguous(), taps=taps, delay=delay, iterations=iterations)[0, ref_ch]
        return y, recorded, chans[ref_ch], fs, filename

    def dereverberate_long(self, original, rir, blind, chunk_seconds=8.0, overlap_seconds=1.0, noise=None, shared_rir=False):
        """Long-form policy (testing/longform.py): one long clean/RIR pair -> the reverberant signal cut into overlapping equal chunks,
        sampled as ONE batch of independent utterances (own operator / RIR estimate each; ``shared_rir``: all chunks form one group of tied
        operator rows, one RIR estimate for the clip), cross-faded back.  Returns (seg, y, pred)."""
        from . import longform
        sr = self.args.exp.sample_rate
        seg, y, _, _ = self.prepare_batch([(original, rir, "long.wav")], blind=False)
        chunk, overlap = int(chunk_seconds * sr), int(overlap_seconds * sr)
        ps = self.args.tester.posterior_sampling
        op_hp = self.args.tester.informed_dereverberation.op_hp

        factory = getattr(self, "noise_factory", None) if noise is None else None
        done = [0]                      # chunks handed out so far: chunk k of the clip is the stream "long_c<k>.wav" however they are batched

        def sample_batch(parts):
            n, clen = parts.shape
            self.sampler.noise = noise(n) if noise is not None else None
            if factory is not None:
                self.sampler.noise = factory([f"long_c{done[0] + k}.wav" for k in range(n)])
                done[0] += n
            if blind:
                op = BlindSubbandFiltering(op_hp, sample_rate=sr, num_utts=n, noise=self.sampler.noise, device=self.device, length=clen,
                                           groups=[0] * n if shared_rir else None)
                op.update_H(use_noise=True)
            else:
                op = RIROperator(op_hp, time_kernel_size=len(rir), sample_rate=sr, device=self.device)
                op.update_params(torch.as_tensor(rir, dtype=torch.float32))
            return self.sampler.predict_conditional(parts.contiguous(), op, shape=(n, clen), blind=blind)

        csm = ps.get("constraint_speech_magnitude", None) if hasattr(ps, "get") else None
        # per-chunk magnitude constraint (blind yaml; an informed run that switches it on is treated alike) -> restore one gain for the clip
        level = bool(csm is not None and csm.get("use", False))
        pred = longform.predict_chunked(sample_batch, y[0], chunk, overlap, level_match=level)
        return seg[0], y[0], pred

    def prepare_directories(self, mode, unconditional=False, blind=False):
        today = date.today()
        self.paths = {}
        if "overriden_name" in self.args.tester.keys() and self.args.tester.overriden_name is not None:
            self.path_sampling = os.path.join(self.args.model_dir, self.args.tester.overriden_name)
        else:
            self.path_sampling = os.path.join(self.args.model_dir, "test" + today.strftime("%d_%m_%Y"))
        self.paths[mode] = os.path.join(self.path_sampling, mode, self.args.exp.exp_name)
        os.makedirs(self.paths[mode], exist_ok=True)
        if not unconditional:
            subs = ["original", "degraded", "reconstructed"]
            if mode == "real_blind_dereverberation":         # no clean signal, no true RIR
                subs = ["degraded", "reconstructed", "estimated_rir"]
                if channel_options(self.args.tester.get("real_recordings", None) or {})[0] == "wpe":
                    subs.append("wpe")              # what the sampler observed: the reference channel after multichannel WPE, or the beamformer's output
                if denoise_options(self.args.tester.get("real_recordings", None) or {})[0]:
                    subs.append("denoised")         # what the sampler observed after the spectral post-filter
            elif "dereverberation" in mode:
                subs.append("true_rir")
                if mode == "blind_dereverberation":
                    subs.append("estimated_rir")
            for s in subs:
                self.paths[mode + s] = os.path.join(self.paths[mode], s)
                os.makedirs(self.paths[mode + s], exist_ok=True)

    def save_experiment_args(self, mode):
        import yaml
        with open(os.path.join(self.paths[mode], ".argv"), "w") as f:
            yaml.safe_dump(_plain(self.args), f)

    def do_test(self, it=0):
        self.it = it
        for m in self.args.tester.modes:
            if m == "unconditional":
                if not self.in_training:
                    self.prepare_directories(m, unconditional=True)
                    self.save_experiment_args(m)
                return self.sample_unconditional(m)
            elif m == "informed_dereverberation":
                if not self.in_training:
                    self.prepare_directories(m)
                    self.save_experiment_args(m)
                self.test_dereverberation(m)
            elif m == "blind_dereverberation":
                if not self.in_training:
                    self.prepare_directories(m)
                    self.save_experiment_args(m)
                self.test_dereverberation(m, blind=True)
            elif m == "real_blind_dereverberation":
                if not self.in_training:
                    self.prepare_directories(m)
                    self.save_experiment_args(m)
                self.test_real_recordings(m)
            else:
                print("Warning: unknown mode: ", m)


def _plain(o):
    if isinstance(o, dict):
        return {k: _plain(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_plain(v) for v in o]
    return o
