#!/usr/bin/env python3
"""Train a DM variant on real wav files at the captured step's rate: corpus on the device, dynamic mixing in one launch per batch
(sepreformer_amd/datafeed.py), ``CapturedTrainStep`` + ``FlatAdamW``, the reference's loss.  Two modes:
``--steps N`` runs N steps at the fixed 0.6 / 0.4 mix and prints the loss and utt/s every ``--log`` steps - a rate check, the weights
are not kept.  ``--epochs N`` runs the reference's training run (``sepreformer_amd/trainer.py``): epochs up to
N - 1 (the reference's ``max_epoch``), each followed by a validation pass over ``--valid-scp``, the warm-up and plateau schedules,
one checkpoint per epoch in ``--checkpoint-dir``, and ``--resume`` to continue from the latest one.

    python tools/train_from_scp.py --form wsj0 --scp s1=tr_s1.scp s2=tr_s2.scp --steps 200
    python tools/train_from_scp.py --form whamr --scp s1=.. s2=.. s1_reverb=.. s2_reverb=.. noise=.. --model SepReformer_Large_DM_WHAMR
    python tools/train_from_scp.py --form wsj0 --scp s1=tr_s1.scp s2=tr_s2.scp --speeds 95:105      # speed perturbation (section 5e-2)
    python tools/train_from_scp.py --form whamr --scp s1=.. s2=.. noise=.. --rir-scp rirs.scp        # reverberation in the launch (section 5e-3)
    python tools/train_from_scp.py --form whamr --scp s1=.. s2=.. noise=.. --synthetic-rirs 64:0.2:0.8
    python tools/train_from_scp.py --form whamr --scp s1=.. s2=.. noise=.. --room-rirs 64:0.2:0.6     # simulated rooms, redrawn per epoch (section 5e-4)
    python tools/train_from_scp.py --form whamr --scp s1=.. s2=.. noise=.. --room-rirs 64:0.2:0.6 --speeds 95:105      # each source perturbed, then reverberated (section 5e-5)
    python tools/train_from_scp.py --form wsj0 --scp s1=tr_s1.scp s2=tr_s2.scp --epochs 200 --valid-scp mix=cv_mix.scp s1=cv_s1.scp s2=cv_s2.scp --checkpoint-dir ck [--resume]
    python tools/train_from_scp.py ... --epochs 200 --valid-scp ... --checkpoint-dir ck --ema-decay 0.999 [--ema-warmup 10] [--validate-with raw|ema|both]      # weight EMA (section 5g-2)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", choices=["wsj0", "wham", "whamr", "direct"], required=True)
    ap.add_argument("--scp", nargs="+", required=True, metavar="ROLE=FILE", help="roles: s1 s2 [mix] [noise] [s1_reverb s2_reverb]")
    ap.add_argument("--model", default="SepReformer_Large_DM_WSJ0")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--max-len", type=int, default=32000)
    ap.add_argument("--fs", type=int, default=8000)
    ap.add_argument("--resample", action="store_true", help="convert files at another rate on the device (default: an error)")
    ap.add_argument("--speeds", default=None, metavar="LO:HI", help="speed perturbation: one speed in percent per source and example, drawn from "
                    "the inclusive range LO:HI or from a comma list (default: off); together with one of the RIR options each source is perturbed first and "
                    "reverberated second, inside the one launch")
    rir = ap.add_mutually_exclusive_group()
    rir.add_argument("--rir-scp", default=None, metavar="FILE", help="reverberation: a 'key path' list of impulse-response wav files; one is drawn per "
                     "source and example and convolved inside the mixing launch (with --form whamr the *_reverb roles are then not needed)")
    rir.add_argument("--synthetic-rirs", default=None, metavar="COUNT:RT60LO:RT60HI", help="reverberation from COUNT synthetic impulse responses "
                     "with RT60 drawn from [RT60LO, RT60HI] seconds (sepreformer_amd.reverb.synthetic_rirs)")
    rir.add_argument("--room-rirs", default=None, metavar="COUNT[:RT60LO:RT60HI]", help="reverberation from COUNT shoebox rooms simulated on the device by the "
                     "image-source method (sepreformer_amd.reverb.RoomSampler; nominal RT60 drawn from [RT60LO, RT60HI] seconds, default 0.2:0.6), "
                     "re-simulated every --rooms-every epochs")
    ap.add_argument("--rooms-every", type=int, default=1, help="with --room-rirs: redraw the rooms at the start of every N-th epoch (default 1)")
    ap.add_argument("--reverb-target", choices=["direct", "dry", "full"], default="direct", help="the targets under reverberation: the direct "
                    "path of the same impulse response (default), the dry source, or the whole response")
    ap.add_argument("--turns", default=None, metavar="LO:HI", help="turn-taking: every source talks for a turn of the example and the turns overlap by a "
                    "fraction drawn per example from [LO, HI] (1 = full overlap, 0 = back to back; default: off); the talker is gated inside the "
                    "mixing launch, before the room")
    ap.add_argument("--turn-ramp", type=int, default=80, metavar="N", help="with --turns: samples of the raised-cosine fade at either end of a turn "
                    "(0 = a hard gate; default 80)")
    ap.add_argument("--turn-absent", type=float, default=0.0, metavar="P", help="with --turns: with probability P one talker of an example, drawn "
                    "uniformly, is silent throughout - its target row is zero (default 0); needs --criterion sasdr")
    ap.add_argument("--conversation-windows", default=None, metavar="COUNT:SECONDS", help="train on windows of --max-len samples cut out of COUNT "
                    "conversations of SECONDS seconds planned anew every epoch (sepreformer_amd.convfeed.ConversationWindowFeed): a varying number "
                    "of utterances per window, talkers who speak twice, more talkers than output channels; the roles s1 s2 are the talkers' "
                    "pool, --form wham / whamr lays the role noise under them as a bed, the room options seat every talker in a room; needs "
                    "--criterion graph_sasdr")
    ap.add_argument("--speakers", type=int, default=3, metavar="N", help="with --conversation-windows: talkers per conversation (default 3)")
    ap.add_argument("--max-active", type=int, default=2, metavar="N", help="with --conversation-windows: talkers who may speak at once, at most the "
                    "model's output channels (default 2)")
    ap.add_argument("--criterion", choices=["sisnr", "sasdr", "graph_sasdr"], default="sisnr", help="the training and validation criteria: the reference's PIT SI-SNR "
                    "pair (default) or the source-aggregated, soft-thresholded SDR pair, which is defined on a silent target (DESIGN.md section 5e-7)")
    ap.add_argument("--snr-max", type=float, default=30.0, metavar="DB", help="with --criterion sasdr: the soft threshold tau = 10^(-DB / 10) (default 30)")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--epochs", type=int, default=None, metavar="N", help="run the epoch loop instead of --steps: the reference's max_epoch "
                    "(epochs 1 .. N - 1); needs --valid-scp and --checkpoint-dir")
    ap.add_argument("--valid-scp", nargs="+", default=None, metavar="ROLE=FILE", help="validation lists: roles mix s1 s2 (fixed mixtures, as the reference validates)")
    ap.add_argument("--test-scp", nargs="+", default=None, metavar="ROLE=FILE", help="test lists (roles mix s1 s2) for the test loop at the reference's test epochs")
    ap.add_argument("--checkpoint-dir", default=None, help="directory of epoch.NNNN.pth files")
    ap.add_argument("--resume", action="store_true", help="continue from the latest checkpoint of --checkpoint-dir (without it a non-empty directory is an error)")
    ap.add_argument("--warmup-steps", type=int, default=1000)
    ap.add_argument("--start-scheduling", type=int, default=50)
    ap.add_argument("--test-epochs", type=int, nargs="*", default=[100, 120, 150, 170], help="epochs after which the test loop runs over --test-scp")
    ap.add_argument("--save", choices=["all", "best"], default="all")
    ap.add_argument("--keep-last", type=int, default=None, help="keep only the N newest checkpoints")
    ap.add_argument("--valid-batch", type=int, default=None, help="validation batch (default: --batch)")
    ap.add_argument("--log", type=int, default=None, help="log interval in steps (default: 10 with --steps; with --epochs the Trainer's own, 50 - each "
                    "log line there is one ledger read-back, a host synchronisation)")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="D", help="with --epochs: keep an exponential moving average of the weights inside "
                    "the optimizer launch (DESIGN.md section 5g-2); the checkpoints then carry ema_state_dict (default: off)")
    ap.add_argument("--ema-warmup", type=float, default=10.0, metavar="W", help="the decay of step t is min(D, (1 + t) / (W + t)); 0 turns the ramp off")
    ap.add_argument("--validate-with", choices=["raw", "ema", "both"], default="ema", help="with --ema-decay: the weights validation, the plateau "
                    "schedule, 'best' and the test loop see (both: two [VALID] lines, the averaged result decides)")
    ap.add_argument("--lr", type=float, default=1.0e-4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    if args.epochs is not None and (not args.valid_scp or not args.checkpoint_dir):
        ap.error("--epochs needs --valid-scp and --checkpoint-dir")
    if args.ema_decay is not None and args.epochs is None:
        ap.error("--ema-decay needs --epochs (the --steps mode keeps no weights)")
    if args.ema_decay is not None and not 0.0 <= args.ema_decay < 1.0:
        ap.error("--ema-decay must lie in [0, 1)")
    if args.speeds and args.form == "direct":
        ap.error("--speeds needs dynamic mixing (--form wsj0, wham or whamr)")
    if args.turns and args.form == "direct":
        ap.error("--turns needs dynamic mixing (--form wsj0, wham or whamr)")
    if args.turn_absent and not args.turns:
        ap.error("--turn-absent needs --turns")
    if not 0.0 <= args.turn_absent <= 1.0:
        ap.error("--turn-absent must lie in [0, 1]")
    if args.turn_absent and args.criterion != "sasdr":
        ap.error("--turn-absent needs --criterion sasdr: the SI-SNR criteria give a zero (time) or exploding (magnitude) gradient on a silent target")
    windows = None
    if args.conversation_windows:
        try:
            count, _, secs = args.conversation_windows.partition(":")
            windows = (int(count), float(secs))
            if windows[0] < 1 or not windows[1] > 0:
                raise ValueError
        except ValueError:
            ap.error("--conversation-windows COUNT:SECONDS, e.g. 32:120")
        if args.form == "direct" or args.speeds or args.turns:
            ap.error("--conversation-windows plans its own conversations: --form wsj0, wham or whamr, without --speeds and --turns")
        if args.reverb_target == "dry":
            ap.error("--conversation-windows: --reverb-target direct or full (a conversation's references are aligned with its mixture)")
        if not 1 <= args.max_active <= args.speakers <= 8:
            ap.error("1 <= --max-active <= --speakers <= 8")
    if (args.criterion == "graph_sasdr") != (windows is not None):
        ap.error("--criterion graph_sasdr and --conversation-windows go together: Graph-PIT assigns the target rows of a window to the channels")
    reverb = args.rir_scp or args.synthetic_rirs or args.room_rirs
    if reverb and args.form == "direct":
        ap.error("--rir-scp / --synthetic-rirs / --room-rirs need dynamic mixing (--form wsj0, wham or whamr)")
    if args.room_rirs:
        from sepreformer_amd.reverb import parse_rooms
        try:
            room_spec = parse_rooms(args.room_rirs)
        except ValueError as e:
            ap.error(f"--room-rirs: {e}")
        if args.rooms_every < 1:
            ap.error("--rooms-every >= 1")
    if args.synthetic_rirs:
        from sepreformer_amd.reverb import parse_synthetic
        try:
            synth = parse_synthetic(args.synthetic_rirs)
        except ValueError as e:
            ap.error(f"--synthetic-rirs: {e}")

    import functools
    import torch
    from sepreformer_amd import datafeed as df
    from sepreformer_amd.config import VARIANTS
    from sepreformer_amd.criterion import PIT_SASDR_mag, PIT_SASDR_time, PIT_SISNR_mag, PIT_SISNR_time
    from sepreformer_amd.model import Model
    from sepreformer_amd.optim import FlatAdamW
    from sepreformer_amd.train_step import CapturedTrainStep

    dev = torch.device(args.device)
    torch.cuda.set_device(dev)
    torch.manual_seed(args.seed)
    corpus = df.Corpus.from_scp(dict(a.split("=", 1) for a in args.scp), fs=args.fs, device=dev, resample=args.resample)
    planner = {"wsj0": df.plan_wsj0, "wham": df.plan_wham, "whamr": df.plan_whamr, "direct": df.plan_direct}[args.form]
    if args.speeds:
        planner = functools.partial(planner, speeds=df.parse_speeds(args.speeds))
    bank = sampler = None
    if reverb:
        from sepreformer_amd.reverb import RirBank, RoomSampler, synthetic_rirs
        if args.rir_scp:
            bank = RirBank.from_scp(args.rir_scp, fs=args.fs, device=dev, resample=args.resample)
        elif args.room_rirs:
            sampler = RoomSampler(rt60=room_spec[1:])
            bank = RirBank.simulate(sampler.draw(room_spec[0], seed=(args.seed, 0)), args.fs, device=dev)      # the feed redraws it per epoch
        else:
            bank = RirBank.from_arrays(synthetic_rirs(synth[0], args.fs, rt60=synth[1:], seed=args.seed), args.fs, device=dev)
        if windows is None:
            planner = functools.partial(planner, rirs=bank, target=args.reverb_target, speed_reverb=bool(args.speeds))
        print(f"RIR bank: {len(bank)} impulse responses, {int(bank.lengths.min())} .. {int(bank.lengths.max())} samples", flush=True)
    if args.turns:
        try:
            planner = functools.partial(planner, turns=df.parse_turns(args.turns, args.turn_ramp),
                                        **({"absent": args.turn_absent} if args.turn_absent else {}))
        except ValueError as e:
            ap.error(f"--turns / --turn-ramp: {e}")
    cfg = VARIANTS[args.model]
    if windows is not None:
        from sepreformer_amd.conversation import plan_conversation
        from sepreformer_amd.convfeed import ConversationWindowFeed
        kw = dict(speakers=args.speakers, max_active=args.max_active)
        if args.form in ("wham", "whamr"):
            kw["noise"] = "noise"
        if bank is not None:
            kw["target"] = args.reverb_target                                 # (simulated rooms are drawn once: this feed does not redraw them)
        try:
            feed = ConversationWindowFeed(corpus, batch=args.batch, max_len=args.max_len, channels=cfg.num_spks, conversations=windows[0],
                                          seconds=windows[1], planner=functools.partial(plan_conversation, **kw), seed=args.seed, rirs=bank)
        except ValueError as e:
            ap.error(f"--conversation-windows: {e}")
    else:
        feed = df.DynamicMixFeed(corpus, planner, batch=args.batch, max_len=args.max_len, seed=args.seed, fixed_length=True, rirs=bank,
                                 rooms=sampler, rooms_every=args.rooms_every)
    print(f"corpus: {len(corpus)} utterances, {corpus.total16 * 2 + corpus.total32 * 4} bytes on {dev}", flush=True)

    model = Model.from_config(cfg, init_seed=args.seed, precision=args.precision).to(dev).train()
    if args.epochs is not None:
        return run_epochs(args, df, model, feed, dev)
    graph = None
    if windows is not None:
        from sepreformer_amd.criterion import GraphPIT
        graph = GraphPIT(dev, cfg.num_spks, feed.rows, args.batch, args.max_len, args.snr_max)
    if args.criterion in ("sasdr", "graph_sasdr"):
        crit_t = PIT_SASDR_time(dev, cfg.num_spks, args.snr_max)
        crit_m = PIT_SASDR_mag(dev, 512, 128, "hann", cfg.num_stages, cfg.num_spks, args.snr_max)
    else:
        crit_t = PIT_SISNR_time(dev, cfg.num_spks, True)
        crit_m = PIT_SISNR_mag(dev, 512, 128, "hann", cfg.num_stages, cfg.num_spks, True, False)
    sizes = torch.full((args.batch,), args.max_len)                           # fixed-length rows: the padding is part of the example
    opt = FlatAdamW(model, lr=args.lr, weight_decay=1.0e-2)

    def loss_fn(audio, aux, *tg):
        tg = list(tg) if graph is None else graph(audio, list(tg))           # Graph-PIT: the channels' targets assembled from the window's rows
        l_time = crit_t(estims=audio, input_sizes=sizes, target_attr=tg)
        l_mag = [crit_m(estims=a, idx=i, input_sizes=sizes, target_attr=tg) for i, a in enumerate(aux)]
        return (0.6 * l_time + 0.4 * sum(l_mag) / len(l_mag)) / cfg.num_spks

    x = torch.zeros(args.batch, args.max_len, device=dev)
    targets = [torch.zeros(args.batch, args.max_len, device=dev) for _ in range(cfg.num_spks if graph is None else feed.rows)]

    def next_into(x, targets):
        plan = feed.next_into(x, targets)
        if graph is not None:
            graph.load(plan.spans, plan.adj)

    next_into(x, targets)
    step = CapturedTrainStep(model, loss_fn, opt, x, targets, max_norm=5.0)
    torch.cuda.synchronize()
    t0, done = time.perf_counter(), 0
    log_every = args.log or 10
    for i in range(1, args.steps + 1):
        next_into(step.x, step.targets)
        loss, gn = step(step.x, step.targets)
        if i % log_every == 0 or i == args.steps:
            val = float(loss.detach())                                        # synchronises: once per log interval
            dt = time.perf_counter() - t0
            print(f"step {i}: loss {val:.4f}  grad norm {float(gn):.3f}  {args.batch * (i - done) / dt:.1f} utt/s", flush=True)
            t0, done = time.perf_counter(), i
    step.release()


def run_epochs(args, df, model, feed, dev):
    """--epochs: the reference's run (sepreformer_amd.trainer.Trainer) on the training feed built above."""
    from sepreformer_amd.trainer import Trainer, latest_checkpoint
    if latest_checkpoint(args.checkpoint_dir) is not None and not args.resume:
        sys.exit(f"{args.checkpoint_dir} holds checkpoints: pass --resume to continue from the latest, or another --checkpoint-dir")
    vcorpus = df.Corpus.from_scp(dict(a.split("=", 1) for a in args.valid_scp), fs=args.fs, device=dev, resample=args.resample)
    vkeys = vcorpus.roles["mix"]
    valid = df.DynamicMixFeed(vcorpus, df.plan_direct, batch=args.valid_batch or args.batch, max_len=args.max_len, seed=args.seed, keys=vkeys,
                              drop_last=False)
    test = None
    if args.test_scp:
        import torch
        from sepreformer_amd.infer import load_audio
        tables = {role: df.parse_scp(path) for role, path in (a.split("=", 1) for a in args.test_scp)}
        srcs = sorted(r for r in tables if r != "mix")

        def test():                                                           # (mixture [1, T], [source_s [1, T]], key), one file at a time
            for key, path in tables["mix"].items():
                yield (torch.from_numpy(load_audio(path)[0])[None].to(dev), [torch.from_numpy(load_audio(tables[r][key])[0])[None].to(dev) for r in srcs],
                       key)
    trainer = Trainer(model, feed, valid, args.checkpoint_dir, lr=args.lr, seed=args.seed, max_epoch=args.epochs, warmup_steps=args.warmup_steps,
                      start_scheduling=args.start_scheduling, test_epochs=args.test_epochs, save=args.save, keep_last=args.keep_last,
                      test_utterances=test, log=lambda s: print(s, flush=True), ema_decay=args.ema_decay, ema_warmup=args.ema_warmup,
                      validate_with=args.validate_with, criterion=args.criterion, snr_max=args.snr_max, **({} if args.log is None else {"log_every": args.log}))
    trainer.run()


if __name__ == "__main__":
    main()
