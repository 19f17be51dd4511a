"""Inference harness with the I/O conventions of the reference's engines.

Mirrors ``models/SepReformer_Base_WSJ0/engine.py``:

* ``separate_file``  - ``Engine._inference_sample`` (:151-172): load a wav at the model's sampling rate, zero-pad
  to a multiple of the encoder stride, run the separator, crop to the input length, write
  ``<name>_in.wav`` and ``<name>_out_<i>.wav`` peak-normalised to 0.9;
* ``evaluate_utterances`` - ``Engine._test`` (:113-149) in full: one utterance per step, device-side ``PIT_SISNRi``
  (eps 1e-15) and ``PIT_SDRi`` (mir_eval's BSS-eval on the CPU in the reference; float64 HIP kernels here), one row per
  utterance in each of the two csv files, running means divided by ``num_spks``, optional ``0.5 / max|.|`` wav dumps;
* ``test_utterances`` - its SI-SNRi half alone (same loop, no SDRi);
* ``evaluate_utterances_all`` - beyond the reference: the same loop with STOI and ESTOI of the estimates beside SI-SNRi and SDRi
  (``criterion.stoi``);
* ``separate_long`` / ``separate_long_file`` - beyond the reference: recordings of any length by overlapping windows of the
  training length, batched through the separator and stitched on the device (``longform.py``);
* ``separate_many_files`` - several files through the stream bank, whose forwards carry one window of every file in flight
  (``streambank.py``);
* ``evaluate_conversations`` / ``score_conversations`` - the test loop of the long-form paths on conversations rendered on the device
  (DESIGN.md section 5h), with ``idle=True`` also what a channel emits while none of its talkers speaks (section 5h-3);
* ``--activity-csv`` on every path that writes tracks: when each separated track carries signal (``activity.channel_activity``).

Host-side logic only; every waveform sample is computed by the HIP separator (``Model.forward``) and the HIP
criterion kernels.  File I/O uses scipy (the reference uses librosa / soundfile, absent here): PCM16/PCM32/float
wavs, multi-channel input averaged to mono as ``librosa.load`` does.  A file at another rate than the model's is converted
on the device when asked to (``resample=True`` / ``--resample``; ``resample.py``), and the outputs can be
written at another rate (``out_rate`` / ``--out-rate``); without the option a rate mismatch raises, as before.
"""
from __future__ import annotations

import csv
import os
from typing import Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .longform import separate_long  # noqa: F401  (re-exported: the long-form entry point)


def _decode(data: np.ndarray) -> np.ndarray:
    if data.dtype == np.int16:
        x = data.astype(np.float32) / 32768.0
    elif data.dtype == np.int32:
        x = (data.astype(np.float64) / 2147483648.0).astype(np.float32)
    elif data.dtype == np.uint8:
        x = (data.astype(np.float32) - 128.0) / 128.0
    else:
        x = data.astype(np.float32)
    if x.ndim == 2:
        x = x.mean(axis=1)
    return np.ascontiguousarray(x)


def load_wav(path: str, fs: int) -> np.ndarray:
    """-> float32 mono in [-1, 1) (``librosa.load(path, sr=fs)`` for a file already at ``fs``)."""
    from scipy.io import wavfile
    sr, data = wavfile.read(path)
    if sr != fs:
        raise RuntimeError(f"{path}: sampling rate {sr} != model rate {fs} (resample the file first)")
    return _decode(data)


def load_audio(path: str) -> Tuple[np.ndarray, int]:
    """-> (float32 mono in [-1, 1), the file's sampling rate): ``load_wav`` without the rate check (``librosa.load(path, sr=None)``)."""
    from scipy.io import wavfile
    sr, data = wavfile.read(path)
    return _decode(data), int(sr)


def pad_to_stride(x: torch.Tensor, stride: int) -> torch.Tensor:
    """Right zero-padding to a multiple of the encoder stride (engine.py:157-163)."""
    remains = x.shape[-1] % stride
    return x if remains == 0 else torch.nn.functional.pad(x, (0, stride - remains), "constant", 0)


def peak_normalise(x: np.ndarray, peak: float) -> np.ndarray:
    """``peak * x / max|x|`` (engine.py:168,171; 0.9 for infer_sample, 0.5 for test_save)."""
    return peak * x / np.max(np.abs(x))


def write_wav(path: str, x: np.ndarray, fs: int) -> None:
    """float waveform -> PCM16 file (soundfile's default subtype for .wav, which the reference relies on).
    libsndfile's float -> short conversion is ``lrint(x * 0x7FFF)`` (normalised floats, round-half-even); the
    same scale is used here so the written files are sample-identical to the reference's ``sf.write`` output
    (the harness peak-normalises to 0.9, reference engine.py:168-172, so nothing clips; the clip is a guard)."""
    from scipy.io import wavfile
    pcm = np.clip(np.rint(np.asarray(x, dtype=np.float64) * 32767.0), -32768, 32767).astype(np.int16)
    wavfile.write(path, fs, pcm)


@torch.no_grad()
def separate(model, mixture: torch.Tensor, stride: Optional[int] = None) -> List[torch.Tensor]:
    """``mixture`` ``[B,T]`` (any T) -> ``num_spks`` tensors ``[B,T]`` on the model's device."""
    stride = stride or model.cfg.enc_stride
    dev = next(model.parameters()).device
    T = mixture.shape[-1]
    x = pad_to_stride(mixture.to(torch.float32), stride).to(dev)
    model.eval()
    audio, _ = model(x)
    return [a[..., :T] for a in audio]


def _load_mixture(model, path: str, fs: int, resample: bool) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """-> (the file's samples, the mixture at ``fs``, the file's rate).  ``resample``: a file at another rate is converted
    to ``fs`` on the model's device; otherwise a mismatch raises (``load_wav``)."""
    if not resample:
        mix = torch.from_numpy(load_wav(path, fs))
        return mix, mix, fs
    from .resample import resample as _resample
    data, sr = load_audio(path)
    mix = torch.from_numpy(data)
    return mix, _resample(mix, sr, fs, device=next(model.parameters()).device), sr


def _write_outputs(model, prefix: str, file_mix: torch.Tensor, sr: int, mix: torch.Tensor, est: Sequence[torch.Tensor], fs: int,
                   out_rate: Union[None, int, str], activity: Optional[dict] = None) -> Tuple[np.ndarray, List[str]]:
    """``<prefix>_in.wav`` and ``<prefix>_out_<i>.wav``, peak-normalised to 0.9, at ``out_rate`` (None: ``fs``; "input": the file's
    rate ``sr``).  The copy of the input is the file's own samples converted from ``sr``; the estimates are converted from ``fs``,
    all of them in one launch.  Returns the raw estimates ``[S,T]`` at ``fs`` as the separator produced them.
    ``activity`` (``{"csv": path, "ratio_db": .., "hang_ms": ..}``): ``activity.channel_activity`` on the estimates at ``fs``, its runs written
    to the csv (``activity.write_activity_csv``: channel, begin s, end s) and the path appended to the files written."""
    from .resample import resample as _resample
    rate = fs if out_rate is None else (sr if out_rate == "input" else int(out_rate))
    dev = next(model.parameters()).device
    copy = mix if rate == fs else _resample(file_mix, sr, rate, device=dev)
    outs = list(est) if rate == fs else _resample([e.contiguous() for e in est], fs, rate, device=dev)
    written = [prefix + "_in.wav"]
    write_wav(written[0], peak_normalise(copy.detach().cpu().numpy(), 0.9), rate)
    for i, o in enumerate(outs):
        written.append(f"{prefix}_out_{i}.wav")
        write_wav(written[-1], peak_normalise(o.detach().cpu().numpy(), 0.9), rate)
    if activity:
        from . import activity as act
        tracks = torch.stack([e.to(dev) for e in est])
        active, _, _ = act.channel_activity(tracks, fs=fs, ratio_db=activity.get("ratio_db", -40.0), hang_ms=activity.get("hang_ms", 200.0))
        act.write_activity_csv(activity["csv"], act.segments(active, act.frame_samples(fs), tracks.shape[1]), fs)
        written.append(activity["csv"])
    return np.stack([e.detach().cpu().numpy() for e in est]), written


def separate_file(model, path: str, fs: int = 8000, out_prefix: Optional[str] = None, resample: bool = False,
                  out_rate: Union[None, int, str] = None, activity: Optional[dict] = None) -> Tuple[np.ndarray, List[str]]:
    """``Engine._inference_sample``.  Returns the raw (un-normalised) estimates ``[S,T]`` at ``fs`` and the files written.
    ``resample``: a file at another rate is converted to ``fs`` on the device before separation (default: it raises).
    ``out_rate``: the estimates and the ``_in.wav`` copy are converted to that rate before peak normalisation and writing
    (``"input"``: the file's own rate; default: ``fs``).  ``activity``: see ``_write_outputs``."""
    file_mix, mix, sr = _load_mixture(model, path, fs, resample)
    est = [e[0] for e in separate(model, mix[None])]
    return _write_outputs(model, out_prefix if out_prefix is not None else path[:-4], file_mix, sr, mix, est, fs, out_rate, activity)


def separate_long_file(model, path: str, fs: int = 8000, out_prefix: Optional[str] = None, chunk_seconds: float = 4.0,
                       overlap_seconds: float = 1.0, match_gain: bool = False, batch: int = 32, resample: bool = False,
                       out_rate: Union[None, int, str] = None, activity: Optional[dict] = None) -> Tuple[np.ndarray, List[str]]:
    """``separate_file`` through ``separate_long``: the same files, the same 0.9 peak normalisation, the same ``resample`` /
    ``out_rate`` options."""
    file_mix, mix, sr = _load_mixture(model, path, fs, resample)
    est = separate_long(model, mix, chunk_seconds=chunk_seconds, overlap_seconds=overlap_seconds, fs=fs, batch=batch,
                        match_gain=match_gain)
    return _write_outputs(model, out_prefix if out_prefix is not None else path[:-4], file_mix, sr, mix, est, fs, out_rate, activity)


def separate_many_files(model, paths: Sequence[str], fs: int = 8000, slots: int = 32, chunk_seconds: float = 4.0,
                        overlap_seconds: float = 1.0, match_gain: bool = False, resample: bool = False,
                        out_rate: Union[None, int, str] = None, activity: Optional[dict] = None) -> List[Tuple[np.ndarray, List[str]]]:
    """``separate_long_file`` for several files at once through ``streambank.separate_many``: per file, the raw estimates and the
    files written (the same names, the same 0.9 peak normalisation, the same ``resample`` / ``out_rate`` options).  With ``resample`` the
    files' own samples and rates go to the bank, which converts every stream inside its hops (``separate_many(rates=...)``): no file is
    converted in a launch and a synchronisation of its own.  The copy of the input is converted only where it is written at ``fs``.
    ``activity``: see ``_write_outputs``; with several files the csv of file ``p`` is named ``<csv root>_<basename of p><csv extension>``."""
    from .streambank import separate_many

    def act_of(p):
        if not activity or len(paths) == 1:
            return activity
        root, ext = os.path.splitext(activity["csv"])
        return {**activity, "csv": f"{root}_{os.path.splitext(os.path.basename(p))[0]}{ext}"}

    if not resample:
        loaded = [_load_mixture(model, p, fs, False) for p in paths]
        ests = separate_many(model, [mix for _, mix, _ in loaded], slots=slots, chunk_seconds=chunk_seconds,
                             overlap_seconds=overlap_seconds, fs=fs, match_gain=match_gain)
        return [_write_outputs(model, p[:-4], file_mix, sr, mix, est, fs, out_rate, act_of(p))
                for p, (file_mix, mix, sr), est in zip(paths, loaded, ests)]
    from .resample import resample as _resample
    files = [(torch.from_numpy(data), sr) for data, sr in map(load_audio, paths)]
    ests = separate_many(model, [x for x, _ in files], slots=slots, chunk_seconds=chunk_seconds, overlap_seconds=overlap_seconds, fs=fs,
                         match_gain=match_gain, rates=[sr for _, sr in files])
    dev = next(model.parameters()).device
    done = []
    for p, (x, sr), est in zip(paths, files, ests):
        at_fs = sr == fs or (fs if out_rate is None else (sr if out_rate == "input" else int(out_rate))) != fs
        done.append(_write_outputs(model, p[:-4], x, sr, x if at_fs else _resample(x, sr, fs, device=dev), est, fs, out_rate, act_of(p)))
    return done


def _test_loop(model, utterances, sisnr_csv_path, sdr_csv_path, wav_dir, fs, with_sdr, stoi_csv_paths=None, stoi_out=None):
    """``Engine._test`` (engine.py:113-149): one utterance per step; PIT_SISNRi (eps 1e-15) and, when ``with_sdr``,
    PIT_SDRi; one csv row per utterance and criterion; running means divided by ``num_spks``; optional wav dumps.
    ``stoi_out`` (a dict, ``evaluate_utterances_all``): STOI and ESTOI of the same estimates as well, one ``criterion.stoi`` call per
    utterance, rows to ``stoi_csv_paths`` = (STOI file, ESTOI file), the running means into the dict."""
    from .criterion import PIT_SDRi, PIT_SISNRi, stoi, stoi_pit
    dev = next(model.parameters()).device
    crit = PIT_SISNRi(dev, model.num_spks, True)
    crit_sdr = PIT_SDRi(dev, 0) if with_sdr else None
    total, total_sdr, n = 0.0, 0.0, 0
    tot_stoi = np.zeros(4)                                                  # STOI, ESTOI, and their improvements over the mixture
    files = [open(p, "w", newline="") if p else None for p in (sisnr_csv_path, sdr_csv_path) + tuple(stoi_csv_paths or (None, None))]
    writers = [csv.writer(fh, quotechar="|", quoting=csv.QUOTE_MINIMAL) if fh else None for fh in files]
    try:
        for mixture, sources, key in utterances:
            if mixture.shape[0] != 1:
                raise RuntimeError("batch size is not one!!")              # engine.py:126-127
            est = separate(model, mixture)
            input_sizes = torch.tensor([mixture.shape[-1]])
            targets = [s.to(dev) for s in sources]
            m, per = crit(estims=est, mixture=mixture.to(dev), input_sizes=input_sizes, target_attr=targets, eps=1.0e-15)
            total += float(m) / model.num_spks
            per_sdr = None
            if crit_sdr is not None:
                m_sdr, per_sdr = crit_sdr(estims=est, mixture=mixture, input_sizes=input_sizes, target_attr=targets)
                total_sdr += m_sdr.item() / model.num_spks
            n += 1
            name = key[:-4] if key.lower().endswith(".wav") else key
            if writers[0]:
                writers[0].writerow([name] + [float(per[i]) for i in range(model.num_spks)])
            if writers[1] and per_sdr is not None:
                writers[1].writerow([name] + [per_sdr[i].item() for i in range(model.num_spks)])
            if stoi_out is not None:
                out = stoi(torch.stack([t[0] for t in targets])[:, None], torch.stack([e[0] for e in est])[:, None],
                           mixture=mixture.to(dev), fs=fs)
                for k, key in enumerate(("stoi", "estoi")):
                    _, val, imp = stoi_pit(out[key].cpu().numpy(), out[key + "_mix"].cpu().numpy())
                    tot_stoi[k] += val[0].sum() / model.num_spks
                    tot_stoi[2 + k] += imp[0].sum() / model.num_spks
                    if writers[2 + k]:
                        writers[2 + k].writerow([name] + [float(v) for v in val[0]])
            if wav_dir:
                os.makedirs(wav_dir, exist_ok=True)
                write_wav(os.path.join(wav_dir, f"{name}{n - 1}_mixture.wav"), peak_normalise(mixture[0].cpu().numpy(), 0.5), fs)
                for i, e in enumerate(est):
                    write_wav(os.path.join(wav_dir, f"{name}{n - 1}_out_{i}.wav"), peak_normalise(e[0].cpu().numpy(), 0.5), fs)
    finally:
        for fh in files:
            if fh:
                fh.close()
    if stoi_out is not None:
        stoi_out.update(zip(("stoi", "estoi", "stoi_i", "estoi_i"), (tot_stoi / n if n else tot_stoi).tolist()))
    return (total / n if n else 0.0), (total_sdr / n if n else 0.0), n


def test_utterances(model, utterances: Iterable[Tuple[torch.Tensor, Sequence[torch.Tensor], str]],
                    csv_path: Optional[str] = None, wav_dir: Optional[str] = None, fs: int = 8000) -> Tuple[float, int]:
    """SI-SNRi loop of ``Engine._test``: ``utterances`` yields ``(mixture [1,T], [source_s [1,T]], key)``.
    Returns (mean SI-SNRi per speaker in dB, number of utterances); writes one csv row per utterance."""
    mean, _, n = _test_loop(model, utterances, csv_path, None, wav_dir, fs, with_sdr=False)
    return mean, n


def evaluate_utterances(model, utterances: Iterable[Tuple[torch.Tensor, Sequence[torch.Tensor], str]],
                        sisnr_csv_path: Optional[str] = None, sdr_csv_path: Optional[str] = None,
                        wav_dir: Optional[str] = None, fs: int = 8000) -> Tuple[float, float, int]:
    """``Engine._test`` in full: ``utterances`` yields ``(mixture [1,T], [source_s [1,T]], key)``.  Returns (mean SI-SNRi
    per speaker, mean SDRi per speaker, number of utterances) in dB; writes one row per utterance to each csv file
    (``test_SISNRi_value.csv`` / ``test_SDRi_value.csv`` in the reference) and the ``0.5 / max|.|`` wav dumps of test_save.
    SDRi rows are indexed by reference source (mir_eval's order), SI-SNRi rows by estimate."""
    return _test_loop(model, utterances, sisnr_csv_path, sdr_csv_path, wav_dir, fs, with_sdr=True)


def evaluate_utterances_all(model, utterances: Iterable[Tuple[torch.Tensor, Sequence[torch.Tensor], str]],
                            sisnr_csv_path: Optional[str] = None, sdr_csv_path: Optional[str] = None,
                            stoi_csv_path: Optional[str] = None, estoi_csv_path: Optional[str] = None,
                            wav_dir: Optional[str] = None, fs: int = 8000) -> dict:
    """``evaluate_utterances`` plus intelligibility: the same loop, the same SI-SNRi and SDRi, and STOI / ESTOI of
    the same estimates on the device.  Returns ``{"sisnri", "sdri", "stoi", "estoi", "stoi_i", "estoi_i", "n"}``: means per speaker over
    the utterances; ``stoi`` / ``estoi`` are the values of the best permutation, ``stoi_i`` / ``estoi_i`` their improvement over the
    mixture.  ``stoi_csv_path`` / ``estoi_csv_path``: one row per utterance, values indexed by reference source, in the csv dialect of
    the other two files."""
    extra: dict = {}
    m_si, m_sdr, n = _test_loop(model, utterances, sisnr_csv_path, sdr_csv_path, wav_dir, fs, with_sdr=True,
                                stoi_csv_paths=(stoi_csv_path, estoi_csv_path), stoi_out=extra)
    return {"sisnri": m_si, "sdri": m_sdr, **extra, "n": n}


test_utterances.__test__ = False      # not a pytest test


def evaluate_conversations(model, corpus, convs, method: str = "long", chunk_seconds: float = 4.0, overlap_seconds: float = 1.0,
                           batch: int = 32, slots: int = 32, match_gain: bool = False, csv_path: Optional[str] = None,
                           wav_dir: Optional[str] = None, fs: int = 8000, rirs=None, idle: bool = False, frame_ms: float = 20.0,
                           collar_seconds: float = 0.25, ratio_db: float = -40.0, hang_ms: float = 200.0,
                           idle_csv_path: Optional[str] = None) -> dict:
    """The test loop of the long-form paths: render every conversation of ``convs`` from the resident ``corpus``
    in one launch (``conversation.render``), separate every mixture with ``separate_long`` (``method="long"``) or
    ``streambank.separate_many`` (``"bank"``), score every output channel against every utterance over that utterance's span
    (``conversation.segment_sisnr``, one call per conversation on views of the flat buffers) and reduce (``conversation.score``).
    Returns that dict - ``sisnri_utt``, ``sisnri_cons``, ``switch_rate``, ``bins`` by overlap fraction, the per-segment vectors - plus
    ``v`` ``[G, C]`` and ``v_mix`` ``[G]`` (numpy) and ``conversations``.  ``csv_path``: one row per segment - conversation key, segment
    number, track, utterance name, begin, length, overlap fraction, best channel, assigned channel (-1 with more talkers than
    channels), ``v_mix``, ``v[0 .. C - 1]`` - in the csv dialect of the test loop.  ``wav_dir``: the mixture and the outputs of every
    conversation, ``0.5 / max|.|`` as ``test_save`` writes them.

    Conversations in rooms or over a noise bed (section 5h-2; ``rirs``: the ``RirBank`` their segments name) are rendered by
    ``sepr_conversation_render_rooms`` and scored against the direct-path tracks of the talkers only; the bed is in the mixture, hence in
    ``v_mix``.  The scored span of a segment moves with the direct path: ``delay = rirs.direct_taps(0.0)[r] - 1`` (0 without a response),
    ``begin = min(place + delay, n - 1)``, ``length = max(1, min(len, n - begin))`` - the csv's ``begin`` and ``length``.

    ``idle=True`` (section 5h-3) also scores what a channel emits while none of its talkers speaks, and gives the assignment that exists
    with more talkers than channels.  ``score`` gets the scored spans, so the dict gains ``coloured``, ``graph``, ``sisnri_graph``,
    ``graph_switch_rate`` and ``bins[*]["sisnri_graph"]``.  The outputs and the mixture are copied into a scratch buffer ``[C + 1][P]`` in
    which every conversation starts on a frame boundary, zeros behind it (zeros add +0.0: every frame has the bits it has alone); ONE
    ``frame_energy`` launch covers it, ``activity.activity_of`` runs per conversation on its ``C`` output rows (a conversation is a
    recording: the level is its own), ``conversation.frame_classes`` classes every frame of every channel from the colouring with a collar
    of ``collar_seconds``, and ``frame_class_sums`` runs once per conversation into one ``[R][C][4][4]`` tensor - the one further copy to
    the host.  Per conversation and channel, ``[R][C]``: ``leak_db = 10 log10((sum_cross e_est + eps) / (sum_cross e_mix + eps))``, NaN
    where class 1 has no frame or no mixture energy, ``quiet_db`` the same over class 2, ``false_alarm`` = active / all frames of the classes
    1 and 2 together, ``miss`` = inactive / all frames of class 0, ``class_frames [R][C][4]``; ``pooled``: the same four figures from the
    energies and counts summed over all conversations and channels BEFORE the logarithm or the division.  ``class_sums [R][C][4][4]``
    (numpy) and ``frames`` - ``frame``, ``collar``, ``hang``, ``offset [R + 1]`` (the first frame of each conversation in ``e``), ``e``
    ``[C + 1][P / frame]`` (device; the last row the mixture), ``active`` and ``classes`` per conversation (device uint8 ``[C][nF_r]``) -
    are what the figures were made from.  ``idle_csv_path``: one row per conversation and channel - key, conversation number, channel, the
    four class counts, ``leak_db``, ``quiet_db``, ``false_alarm``, ``miss``.  With ``idle=False`` nothing of this runs."""
    from . import conversation as cv
    if method not in ("long", "bank"):
        raise ValueError(f"method must be 'long' or 'bank', got {method!r}")
    convs = list(convs)
    rd = cv.render(corpus, convs, tracks=True, rirs=rirs)
    mixes = [rd.mixture(r) for r in range(len(convs))]
    if method == "long":
        ests = separate_long(model, mixes, chunk_seconds=chunk_seconds, overlap_seconds=overlap_seconds, fs=fs, batch=batch,
                             match_gain=match_gain)
    else:
        from .streambank import separate_many
        ests = separate_many(model, mixes, slots=slots, chunk_seconds=chunk_seconds, overlap_seconds=overlap_seconds, fs=fs,
                             match_gain=match_gain)
    C = model.num_spks
    out = score_conversations(corpus, convs, rd, ests, C, csv_path=csv_path, fs=fs, rirs=rirs, idle=idle, frame_ms=frame_ms,
                              collar_seconds=collar_seconds, ratio_db=ratio_db, hang_ms=hang_ms, idle_csv_path=idle_csv_path)
    if wav_dir:
        os.makedirs(wav_dir, exist_ok=True)
        for r, conv in enumerate(convs):
            name = conv.key.replace("/", "_")
            write_wav(os.path.join(wav_dir, f"{name}{r}_mixture.wav"), peak_normalise(mixes[r].cpu().numpy(), 0.5), fs)
            for c in range(C):
                write_wav(os.path.join(wav_dir, f"{name}{r}_out_{c}.wav"), peak_normalise(ests[r][c].cpu().numpy(), 0.5), fs)
    return out


def score_conversations(corpus, convs, rd, ests, C: int, csv_path: Optional[str] = None, fs: int = 8000, rirs=None, idle: bool = False,
                        frame_ms: float = 20.0, collar_seconds: float = 0.25, ratio_db: float = -40.0, hang_ms: float = 200.0,
                        idle_csv_path: Optional[str] = None) -> dict:
    """The scoring half of ``evaluate_conversations``, whose arguments these are: ``rd`` the rendered conversations (``conversation.render``
    with tracks), ``ests[r]`` the ``C`` output rows ``[n_r]`` of conversation ``r`` on the device, however they were made."""
    from . import conversation as cv
    convs = list(convs)
    peak = rirs.direct_taps(0.0) if rirs is not None else None
    spans = []                                                    # per conversation: its talker segments, their scored begin and length
    for conv in convs:
        k = np.nonzero(conv.track < conv.S)[0]
        delay = np.zeros(len(k), dtype=np.int64)
        if conv.rir is not None and peak is not None:
            wet = conv.rir[k] >= 0
            delay[wet] = peak[conv.rir[k][wet]] - 1
        begin = np.minimum(conv.place[k].astype(np.int64) + delay, conv.n - 1)
        spans.append((k, begin.astype(np.int32), np.maximum(1, np.minimum(conv.len[k], conv.n - begin)).astype(np.int32)))
    est_all = torch.empty(C, rd.table.total, dtype=torch.float32, device=rd.mix.device)      # the row stride of the tracks: no repacking below
    vs, vms = [], []
    for r, (conv, est) in enumerate(zip(convs, ests)):
        a, b = int(rd.out_off[r]), int(rd.out_off[r + 1])
        for c in range(C):
            est_all[c, a:b].copy_(est[c])
        k, begin, length = spans[r]
        v, v_mix = cv.segment_sisnr(est_all[:, a:b], rd.tracks_of(r), rd.mixture(r), conv.track[k], begin, length)
        vs.append(v)
        vms.append(v_mix)
    v, v_mix = torch.cat(vs).cpu().numpy(), torch.cat(vms).cpu().numpy()                      # the one copy of the scores
    conv_of = np.concatenate([np.full(len(k), r) for r, (k, _, _) in enumerate(spans)])
    out = cv.score(v, v_mix, conv_of, np.concatenate([c.track[k] for c, (k, _, _) in zip(convs, spans)]), [c.S for c in convs], C,
                   overlap=np.concatenate([cv.overlap_fraction(c)[k] for c, (k, _, _) in zip(convs, spans)]),
                   spans=(np.concatenate([b for _, b, _ in spans]), np.concatenate([n for _, _, n in spans])) if idle else None)
    out.update(v=v, v_mix=v_mix, conversations=len(convs))
    if idle:
        from . import activity as act
        frame, hang, collar = act.frame_samples(fs, frame_ms), act.hang_frames(frame_ms, hang_ms), int(round(float(collar_seconds) * fs))
        offset = np.concatenate([[0], np.cumsum([-(-int(c.n) // frame) for c in convs])]).astype(np.int64)
        pad = torch.zeros(C + 1, int(offset[-1]) * frame, dtype=torch.float32, device=rd.mix.device)      # conversations on frame boundaries
        for r, conv in enumerate(convs):
            a, p = int(rd.out_off[r]), int(offset[r]) * frame
            pad[:C, p:p + conv.n].copy_(est_all[:, a:a + conv.n])
            pad[C, p:p + conv.n].copy_(rd.mixture(r))
        e = act.frame_energy(pad, frame)                                                                  # ONE launch: every row, every frame
        sums = torch.empty(len(convs), C, 4, 4, dtype=torch.float64, device=e.device)
        actives, classes, g = [], [], 0
        for r, (conv, (k, begin, length)) in enumerate(zip(convs, spans)):
            fa, fb = int(offset[r]), int(offset[r + 1])
            e_est = e[:C, fa:fb].contiguous()
            active, _ = act.activity_of(e_est, ratio_db=ratio_db, hang=hang)
            cls = torch.from_numpy(cv.frame_classes((begin, length), out["coloured"][g:g + len(k)], conv.n, C, frame, collar)).to(e.device)
            act.frame_class_sums(e_est, e[C, fa:fb], active, cls, out=sums[r])
            actives.append(active)
            classes.append(cls)
            g += len(k)
        sums_h = sums.cpu().numpy()                                                                       # the one copy of the idle sums
        out.update(cv.idle_figures(sums_h))
        pooled = cv.idle_figures(sums_h.reshape(-1, 4, 4).sum(axis=0))                                    # energies and counts first, then the log
        out.update(class_frames=sums_h[..., 0].astype(np.int64), class_sums=sums_h, pooled={key: float(x) for key, x in pooled.items()},
                   frames={"frame": frame, "collar": collar, "hang": hang, "offset": offset, "e": e, "active": actives, "classes": classes})
        if idle_csv_path:
            with open(idle_csv_path, "w", newline="") as fh:
                w = csv.writer(fh, quotechar="|", quoting=csv.QUOTE_MINIMAL)
                for r, conv in enumerate(convs):
                    for c in range(C):
                        w.writerow([conv.key, r, c] + [int(x) for x in out["class_frames"][r, c]] +
                                   [float(out[key][r, c]) for key in ("leak_db", "quiet_db", "false_alarm", "miss")])
    if csv_path:
        with open(csv_path, "w", newline="") as fh:
            w = csv.writer(fh, quotechar="|", quoting=csv.QUOTE_MINIMAL)
            g = 0
            for conv, (ks, begin, length) in zip(convs, spans):
                for i, k in enumerate(ks):
                    w.writerow([conv.key, int(k), int(conv.track[k]), corpus.names[int(conv.utt[k])], int(begin[i]), int(length[i]),
                                float(out["overlap"][g]), int(out["best"][g]), int(out["assigned"][g]), float(v_mix[g])] +
                               [float(x) for x in v[g]])
                    g += 1
    return out


def load_checkpoint_weights(model, path: str, ema: bool = False):
    """The weights of a checkpoint - the reference's, or one ``trainer.Trainer`` wrote (the same five keys) - or of a bare state dict.
    ``ema=True``: the averaged weights a ``Trainer(ema_decay=...)`` run saved beside them (``ema_state_dict``: the same keys, parameters
    from the average, buffers from the model); a file without them is a ``ValueError``."""
    ck = torch.load(path, map_location="cpu")
    if ema:
        if "ema_state_dict" not in ck:
            raise ValueError(f"{path} holds no ema_state_dict (it was written without a weight EMA): load it without ema")
        return model.load_state_dict(ck["ema_state_dict"], strict=False)
    return model.load_state_dict(ck.get("model_state_dict", ck), strict=False)      # utils/util_engine.py:43


def _main() -> None:
    import argparse
    from .config import VARIANTS
    from .model import Model
    ap = argparse.ArgumentParser(description="separate one wav file (reference: run.py --engine-mode infer_sample), or several "
                                             "through the stream bank")
    ap.add_argument("wav", nargs="+")
    ap.add_argument("--model", default="SepReformer_Base_WSJ0", choices=sorted(VARIANTS))
    ap.add_argument("--checkpoint", default=None, help="reference checkpoint (.pth with model_state_dict); default: synthetic weights")
    ap.add_argument("--ema", action="store_true", help="with --checkpoint: load the averaged weights (ema_state_dict) a run with a weight EMA saved")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--chunk-seconds", type=float, default=None,
                    help="long-form mode: overlapping windows of this length, stitched on the device (default: one whole-file forward)")
    ap.add_argument("--overlap-seconds", type=float, default=1.0, help="long-form mode: overlap of consecutive windows")
    ap.add_argument("--batch", type=int, default=32, help="long-form mode: windows of the recording per forward")
    ap.add_argument("--slots", type=int, default=None,
                    help="stream-bank mode (implied by several files): files in flight at once, one window of each per forward; "
                         "windows of --chunk-seconds (default 4)")
    ap.add_argument("--match-gain", action="store_true", help="long-form mode: align each speaker track's gain across windows")
    ap.add_argument("--resample", action="store_true",
                    help="convert a file at another sampling rate to the model's rate on the device (default: such a file is an error)")
    ap.add_argument("--out-rate", default=None, metavar="{N,input}",
                    help="write the outputs at N Hz, or at the input file's own rate (default: the model's rate)")
    ap.add_argument("--activity-csv", default=None, metavar="OUT",
                    help="also write when each separated track carries signal: one row per run of active 20 ms frames - channel, begin s, "
                         "end s - at the model's rate (several files: OUT gains _<file name> before its extension)")
    ap.add_argument("--activity-ratio-db", type=float, default=-40.0,
                    help="--activity-csv: a frame is active above this level relative to the track's loudest frame (a convention, not a tuned value)")
    ap.add_argument("--activity-hang-ms", type=float, default=200.0, help="--activity-csv: an active frame keeps its neighbours within this time active")
    args = ap.parse_args()
    activity = {"csv": args.activity_csv, "ratio_db": args.activity_ratio_db, "hang_ms": args.activity_hang_ms} if args.activity_csv else None
    out_rate = args.out_rate if args.out_rate in (None, "input") else int(args.out_rate)
    model = Model.from_config(VARIANTS[args.model], init_seed=0)
    if args.ema and not args.checkpoint:
        ap.error("--ema needs --checkpoint")
    if args.checkpoint:
        try:
            load_checkpoint_weights(model, args.checkpoint, ema=args.ema)
        except ValueError as e:
            if not args.ema:
                raise
            raise SystemExit(str(e))                     # a file without the averaged weights: the message, status 1
    else:
        model.load_synthetic_(0)
    model = model.eval().to(args.device)
    if len(args.wav) > 1 or args.slots is not None:
        done = separate_many_files(model, args.wav, slots=32 if args.slots is None else args.slots,
                                   chunk_seconds=4.0 if args.chunk_seconds is None else args.chunk_seconds,
                                   overlap_seconds=args.overlap_seconds, match_gain=args.match_gain, resample=args.resample,
                                   out_rate=out_rate, activity=activity)
        written = [w for _, ws in done for w in ws]
    elif args.chunk_seconds is None:
        _, written = separate_file(model, args.wav[0], resample=args.resample, out_rate=out_rate, activity=activity)
    else:
        _, written = separate_long_file(model, args.wav[0], chunk_seconds=args.chunk_seconds, overlap_seconds=args.overlap_seconds,
                                        match_gain=args.match_gain, batch=args.batch, resample=args.resample, out_rate=out_rate, activity=activity)
    print("\n".join(written))


if __name__ == "__main__":
    _main()
