#!/usr/bin/env python3
"""Score long-form separation on conversations rendered on the device (infer.evaluate_conversations).

The utterances of the scp lists are loaded into a device-resident ``Corpus``; COUNT conversations of MINUTES minutes are planned from them
(``conversation.plan_conversation``, seed = the conversation's number), rendered in one launch, separated with ``separate_long``
(``--method long``) or the stream bank (``--method bank``) and scored per utterance: SI-SNRi of the best channel per utterance, SI-SNRi
under the one consistent track -> channel assignment, the rate of channel switches, all three also by overlap ratio.

    python tools/eval_conversations.py --scp s1=tt_s1.scp s2=tt_s2.scp --count 20 --minutes 10 --overlap 0:0.4 --method bank [--checkpoint F [--ema]]

Rooms and noise (section 5h-2), for the models trained on reverberant or noisy mixtures: every talker of a conversation sits in one room of a bank
(``--rir-scp``, ``--synthetic-rirs`` or ``--room-rirs``, as ``tools/train_from_scp.py`` takes them) and is scored against the direct path of their
own voice; ``--noise-role`` lays the utterances of that role end to end under the whole conversation.

    python tools/eval_conversations.py --scp s1=tt_s1.scp s2=tt_s2.scp noise=tt_noise.scp --noise-role noise --room-rirs 64:0.2:0.6 --model SepReformer_Large_DM_WHAMR

Idle channels (section 5h-3): ``--idle`` adds the colouring-based assignment, which exists with more talkers than channels too, and what a channel
emits in the frames none of its talkers owns - the pooled leak over the other talkers' frames, over quiet frames, the false-alarm and the miss rate
of the activity detector.

    python tools/eval_conversations.py --scp s1=tt_s1.scp s2=tt_s2.scp --speakers 3 --max-active 2 --idle --idle-csv idle.csv
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _range(text, what):
    lo, _, hi = text.partition(":")
    try:
        return float(lo), float(hi if hi else lo)
    except ValueError:
        raise SystemExit(f"{what}: expected LO:HI, got {text!r}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scp", nargs="+", required=True, metavar="ROLE=FILE", help="utterance lists, one role per talker position: s1=... s2=...")
    ap.add_argument("--count", type=int, default=20, help="conversations")
    ap.add_argument("--minutes", type=float, default=10.0, help="length of each conversation")
    ap.add_argument("--speakers", type=int, default=2, help="talker tracks per conversation (more than the model's channels: score them with --idle)")
    ap.add_argument("--overlap", default="0:0.4", metavar="LO:HI", help="overlap of a turn with the one before, as a share of the shorter utterance")
    ap.add_argument("--pause", default="0:1", metavar="LO:HI", help="seconds between turns that do not overlap")
    ap.add_argument("--p-overlap", type=float, default=0.5, help="probability that a turn overlaps the one before")
    ap.add_argument("--max-active", type=int, default=2, help="talkers active at once, at most")
    ap.add_argument("--method", choices=["long", "bank"], default="long")
    ap.add_argument("--chunk-seconds", type=float, default=4.0)
    ap.add_argument("--overlap-seconds", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=32, help="--method long: windows per forward")
    ap.add_argument("--slots", type=int, default=32, help="--method bank: conversations in flight")
    ap.add_argument("--match-gain", action="store_true")
    ap.add_argument("--model", default="SepReformer_Base_WSJ0")
    ap.add_argument("--checkpoint", default=None, help="checkpoint (.pth with model_state_dict); default: synthetic weights")
    ap.add_argument("--ema", action="store_true", help="with --checkpoint: the averaged weights a run with a weight EMA saved")
    ap.add_argument("--fs", type=int, default=8000)
    ap.add_argument("--resample", action="store_true", help="convert files at another rate on the device (default: an error)")
    ap.add_argument("--device", default="cuda:0")
    rir = ap.add_mutually_exclusive_group()
    rir.add_argument("--rir-scp", default=None, metavar="FILE", help="rooms: a 'key path' list of impulse-response wav files; one is drawn per talker "
                     "and conversation and convolved inside the render launch")
    rir.add_argument("--synthetic-rirs", default=None, metavar="COUNT:RT60LO:RT60HI", help="rooms from COUNT synthetic impulse responses with RT60 "
                     "drawn from [RT60LO, RT60HI] seconds (sepreformer_amd.reverb.synthetic_rirs)")
    rir.add_argument("--room-rirs", default=None, metavar="COUNT[:RT60LO:RT60HI]", help="rooms from COUNT shoebox rooms simulated on the device by the "
                     "image-source method (sepreformer_amd.reverb.RoomSampler; default RT60 range 0.2:0.6)")
    ap.add_argument("--reverb-target", choices=["direct", "full"], default="direct", help="the scoring reference of a talker in a room: the direct "
                    "path of their response (default) or the whole response")
    ap.add_argument("--early-ms", type=float, default=0.0, help="with --reverb-target direct: this much of the early reflections counts as direct")
    ap.add_argument("--noise-role", default=None, metavar="ROLE", help="a noise bed under every conversation from the utterances of this --scp role")
    ap.add_argument("--noise-db", default="-6:3", metavar="LO:HI", help="the bed's gain is 10^(-u / 20), u uniform in [LO, HI] dB (one draw per conversation); "
                    "write a negative LO as --noise-db=-6:3")
    ap.add_argument("--seed", type=int, default=0, help="seed of the synthetic or simulated rooms")
    ap.add_argument("--csv", default=None, help="one row per utterance of every conversation")
    ap.add_argument("--wav-dir", default=None, help="write every mixture and every output channel")
    ap.add_argument("--idle", action="store_true", help="also score idle channels (DESIGN.md section 5h-3): the colouring-based assignment that "
                    "exists for any number of talkers, and what a channel emits in the frames none of its talkers owns")
    ap.add_argument("--collar", type=float, default=0.25, help="--idle: seconds around a channel's own utterances that count as neither own nor idle")
    ap.add_argument("--frame-ms", type=float, default=20.0, help="--idle: the frame of the activity measure")
    ap.add_argument("--idle-csv", default=None, help="--idle: one row per conversation and channel")
    args = ap.parse_args()
    if args.idle_csv and not args.idle:
        ap.error("--idle-csv needs --idle")
    if args.ema and not args.checkpoint:
        ap.error("--ema needs --checkpoint")
    scps = {}
    for item in args.scp:
        role, eq, path = item.partition("=")
        if not eq or not role or not path:
            ap.error(f"--scp takes ROLE=FILE, got {item!r}")
        scps[role] = path
    if args.noise_role is not None and args.noise_role not in scps:
        ap.error(f"--noise-role {args.noise_role}: no such role among --scp")
    from sepreformer_amd import reverb
    try:
        room_spec = reverb.parse_rooms(args.room_rirs) if args.room_rirs else None
        synth = reverb.parse_synthetic(args.synthetic_rirs) if args.synthetic_rirs else None
    except ValueError as e:
        ap.error(f"--room-rirs / --synthetic-rirs: {e}")
    from sepreformer_amd import conversation as cv
    from sepreformer_amd import infer
    from sepreformer_amd.config import VARIANTS
    from sepreformer_amd.datafeed import Corpus
    from sepreformer_amd.model import Model
    model = Model.from_config(VARIANTS[args.model], init_seed=0)
    if args.checkpoint:
        infer.load_checkpoint_weights(model, args.checkpoint, ema=args.ema)
    else:
        model.load_synthetic_(0)
    model = model.eval().to(args.device)
    corpus = Corpus.from_scp(scps, fs=args.fs, device=args.device, resample=args.resample)
    bank = None
    if args.rir_scp:
        bank = reverb.RirBank.from_scp(args.rir_scp, fs=args.fs, device=args.device, resample=args.resample)
    elif room_spec:
        bank = reverb.RirBank.simulate(reverb.RoomSampler(rt60=room_spec[1:]).draw(room_spec[0], seed=(args.seed, 0)), args.fs, device=args.device)
    elif synth:
        bank = reverb.RirBank.from_arrays(reverb.synthetic_rirs(synth[0], args.fs, rt60=synth[1:], seed=args.seed), args.fs, device=args.device)
    talkers = tuple(r for r in scps if r != args.noise_role)
    convs = [cv.plan_conversation(corpus, random.Random(i), seconds=60.0 * args.minutes, roles=talkers, speakers=args.speakers,
                                  overlap=_range(args.overlap, "--overlap"), pause=_range(args.pause, "--pause"), p_overlap=args.p_overlap,
                                  max_active=args.max_active, key=f"conv{i:03d}", rirs=bank, target=args.reverb_target, early_ms=args.early_ms,
                                  noise=args.noise_role, noise_db=_range(args.noise_db, "--noise-db")) for i in range(args.count)]
    out = infer.evaluate_conversations(model, corpus, convs, method=args.method, chunk_seconds=args.chunk_seconds,
                                       overlap_seconds=args.overlap_seconds, batch=args.batch, slots=args.slots, match_gain=args.match_gain,
                                       csv_path=args.csv, wav_dir=args.wav_dir, fs=args.fs, rirs=bank, idle=args.idle, frame_ms=args.frame_ms,
                                       collar_seconds=args.collar, idle_csv_path=args.idle_csv)
    summary = {"method": args.method, "conversations": out["conversations"], "utterances": out["n"], "sisnri_utt": out["sisnri_utt"],
               "sisnri_cons": out["sisnri_cons"], "switch_rate": out["switch_rate"], "bins": out["bins"]}
    if args.idle:
        summary.update(sisnri_graph=out["sisnri_graph"], graph_switch_rate=out["graph_switch_rate"], **out["pooled"])
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
