#!/usr/bin/env python3
"""Benchmark of the DFCNN(+SE)+CTC training hot path on MI355X.

A "step" = one pass of the hot path over one batch of synthetic 10 s / 16 kHz utterances
that are already resident in HBM as raw audio:
    fbank (K1) -> DFCNN forward -> softmax/log -> CTC loss+grad, greedy decode, edit distance
    -> backward (dgrad + wgrad of every layer) -> [RCCL gradient all-reduce] -> TF-Adam.
Workloads (BASELINE.json configs):
    dfcnn     configs[1]: plain DFCNN  lm_and_am/model/acoustic_model.py,  batch 32, T_pad 1600  (default)
    se_dfcnn  configs[2]: SE-DFCNN     lm_and_am/model/acoustic_model2.py, batch 32 per GPU
Prints ONE JSON line (rank 0).  `python bench.py` = 1 GPU, a few minutes incl. the CPU baseline.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.distributed as dist

FP32_PEAK_TFLOPS = 157.3        # MI355X dense fp32 (vector = matrix), MI355X_MICROARCH.md


# Winograd kernels (wino.hip F(2x2,3x3) forward / data-gradient, wino_wgrad.hip F(3x3,2x2) weight gradient): 16 instead of 36
# multiplies per 2x2 tile and channel pair.  SURVEY 8d counts a conv layer in the flops of the DIRECT convolution; a Winograd
# kernel EXECUTES 1/2.25 of them on the fp32 matrix pipe.  The roofline of such a kernel is priced in executed flops against
# the plain fp32 MFMA peak (round 5): `achieved` = direct-conv flops / 2.25 / duration, `peak` = 157.3,
# `frac` = achieved / peak -- what PMC's SQ_VALU_MFMA_BUSY_CYCLES shows as pipe occupancy, to within the clock (157.3 TFLOP/s
# assumes 2.4 GHz, the chip runs these kernels at 2.2-2.35).  The direct-conv rate (the rate of useful work, which can exceed
# 157.3) stays in the line as `achieved_direct`.  Rounds 3-4 priced these kernels against 157.3 x 2.25 x 0.91 (0.91 = the
# measured MFMA time share of the FORWARD kernel's issue pattern); that factor was never measured for the weight gradient.
WINO_MULT_SAVING = 2.25


def kernel_peak(sym):
    """(peak TFLOP/s, executed flops per algorithmic flop, explanation or None)."""
    if sym.startswith('wino'):
        return (FP32_PEAK_TFLOPS, 1.0 / WINO_MULT_SAVING,
                'Winograd in fp32 (F(2x2,3x3) forward / data-gradient, F(3x3,2x2) weight gradient): the kernel executes 1/2.25 of the '
                'multiplies of the direct 3x3 convolution; `achieved` / `frac` count the EXECUTED flops against the fp32 MFMA peak, '
                '`achieved_direct` is the rate in direct-convolution flops (SURVEY 8d: 2 x MACs)')
    return FP32_PEAK_TFLOPS, 1.0, None


def is_forward_symbol(sym):
    """Contraction kernels that only the forward pass launches (they run alone on the main stream even when the backward
    pass uses two): wino11_kernel<DIR, EPI> / wino8_kernel<DIR>, tap_gemm_kernel_v5<..., DIR>, tap_gemm_kernel_v1<MT, NT, WM, WN, NTAPS, WMODE[, KC]>,
    gemm1_kernel<DIR, NB> with DIR / WMODE 0."""
    if '<' not in sym:
        return False
    args = [a.strip() for a in sym[sym.index('<') + 1:sym.rindex('>')].split(',')]
    if sym.startswith('wino8_kernel') or sym.startswith('wino11_kernel'):
        return args[0] == '0'
    if sym.startswith('gemm1_kernel'):
        return args[0] == '0'
    if sym.startswith('tap_gemm_kernel_v5'):
        return args[-1] == '0'
    if sym.startswith('tap_gemm_kernel_v1'):
        return args[5] == '0'
    return False


def roofline_block(dom, r, steps):
    """The `roofline` object for kernel symbol `dom` from its KernelTimer record r (HIP events on the launch stream)."""
    peak, executed, why = kernel_peak(dom)
    ach = r['tflops'] * executed
    out = {'bound': 'mfma', 'achieved': round(ach, 2), 'peak': peak, 'unit': 'TFLOP/s',
           'frac': round(ach / peak, 4), 'traffic': None, 'kernel': dom,
           'launches_per_step': r['launches'] // max(1, steps), 'avg_launch_us': round(r['avg_us'], 2),
           'flop_per_launch': round(r['total_flops'] * executed / r['launches'] / 1e9, 3), 'flop_unit': 'GFLOP (executed)'}
    if why:
        out['peak_note'] = why
        out['achieved_direct'] = round(r['tflops'], 2)
        out['flop_per_launch_direct'] = round(r['total_flops'] / r['launches'] / 1e9, 3)
    return out


def pmc_traffic(workload, symbol):
    """HBM bytes per launch of `symbol` from the latest committed PMC pass (profiles/*_<workload>_traffic.json,
    written from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE runs with the gfx950 x2 FETCH correction of
    MI355X_MICROARCH.md).  Returns (bytes or None, source file or None)."""
    import glob
    tag = {'dfcnn': 'dfcnn_m1', 'se_dfcnn': 'se_dfcnn_m2'}.get(workload, workload)
    files = sorted(glob.glob(os.path.join(ROOT, 'profiles', '*_%s_traffic.json' % tag)))
    if not files:
        return None, None
    try:
        d = json.load(open(files[-1]))
        return (d[symbol]['hbm_bytes_per_launch'] if symbol in d else None), os.path.relpath(files[-1], ROOT)
    except Exception:
        return None, None


def attach_traffic(out, workload, dom, default_config):
    """roofline.traffic = HBM bytes per launch of the dominant kernel from the committed PMC pass of this workload (null when
    the run is not the configuration that pass was taken on)."""
    tr, src = pmc_traffic(workload, dom) if default_config else (None, None)
    out['roofline']['traffic'] = tr
    if src:
        out['roofline']['traffic_unit'] = 'bytes/launch (PMC pass: %s)' % src


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays, limit=DUMP_LIMIT_BYTES, seed=0):
    """--dump-outputs: writes every tensor of ``arrays`` ({name: tensor}) as out_dir/<name>.npy, float64 as float64 and everything
    else as float32 (the integer outputs -- ids, lengths -- are far below 2**24, so exact), for comparing two builds output for output.
    At most ``limit`` bytes in all: taken from the smallest to the largest, an array larger than an equal share of the bytes still
    free is written as a fixed sample of its elements instead, the 1-D array flat[np.sort(default_rng(seed).choice(n, k, replace=False))]
    -- the same elements in every run of the same shape.  Returns {name: (shape, elements written)}."""
    os.makedirs(out_dir, exist_ok=True)
    items = sorted(((name, t.detach(), 8 if t.dtype == torch.float64 else 4) for name, t in arrays.items()),
                   key=lambda it: it[1].numel() * it[2])
    free = limit - 256 * len(items)                       # the .npy headers (128 bytes for these shapes)
    written = {}
    for i, (name, t, size) in enumerate(items):
        n, share = t.numel(), free // (len(items) - i)
        flat = t.reshape(-1)
        if n * size > share:
            idx = np.sort(np.random.default_rng(seed).choice(n, share // size, replace=False))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        a = flat.to(torch.float64 if size == 8 else torch.float32).cpu().numpy()
        np.save(os.path.join(out_dir, name + '.npy'), a.reshape(t.shape) if a.size == n else a)
        free -= a.nbytes
        written[name] = (tuple(t.shape), a.size)
    total = sum(os.path.getsize(os.path.join(out_dir, name + '.npy')) for name in written)
    assert total <= limit, (total, limit)
    for name, (shape, k) in written.items():
        n = int(np.prod(shape))
        print('bench.py: --dump-outputs %s/%s.npy: %s%s' % (out_dir, name, shape, '' if k == n else ', sample of %d of %d elements' % (k, n)),
              file=sys.stderr)
    return written


def decoded_ids(ids, lens):
    """greedy-decode ids [B][T] with -1 behind each row's decoded length (the buffer's tail is not part of the result)"""
    cols = torch.arange(ids.shape[1], device=ids.device)
    return torch.where(cols[None, :] < lens[:, None], ids, torch.full_like(ids, -1))


def cpu_baseline(variant, t_pad, vocab, batch=32, seconds=10.0, budget_s=30.0):
    """CPU restatement ("port": oracle/torch_ref.py on torch-CPU ops + the numpy fbank oracle) of the identical step at the
    SAME batch the GPU number is quoted on, timed on this host's cores on a bounded sample: one untimed warm-up
    step, then timed steps until `budget_s` is used up (at least one).  Stand-in for the reference's TF-CPU path, which
    cannot run offline."""
    from oracle import dfcnn as odf, fbank as ofb, torch_ref
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = max(1, min(cores, 64))
    torch.set_num_threads(cores)
    Bc = batch
    g = odf.graph(variant, vocab)
    P = odf.init_params(g, seed=0)
    tP = torch_ref.to_torch_params(P, dtype=torch.float32)
    params = [t for d in tP.values() for t in d.values()]
    m = [torch.zeros_like(p) for p in params]
    v = [torch.zeros_like(p) for p in params]
    rng = np.random.default_rng(1234)
    ns = int(seconds * 16000)
    sig = [0.1 * rng.standard_normal(ns) for _ in range(Bc)]
    labels = [list(rng.integers(1, vocab - 1, 32)) for _ in range(Bc)]

    def step(t):
        x = np.zeros((Bc, t_pad, 200, 1), dtype=np.float32)
        for b in range(Bc):
            f = ofb.compute_fbank_from_api(sig[b], 16000, nfilt=200)
            x[b, :f.shape[0], :, 0] = f
        for p in params:
            p.grad = None
        torch_ref.train_step(g, tP, torch.from_numpy(x), [125] * Bc, labels)
        torch_ref.adam_tf_(params, [p.grad for p in params], m, v, 7e-4, t)

    tw = time.perf_counter()
    step(1)                                   # warm-up (allocations, oneDNN primitive caches)
    tw = time.perf_counter() - tw
    n, t0 = 0, time.perf_counter()
    while True:
        step(n + 2)
        n += 1
        el = time.perf_counter() - t0
        if el + el / n > budget_s or n >= 10:
            break
    return {'value': round(Bc * n / el, 4), 'unit': 'utterances/s', 'cores': cores, 'kind': 'port',
            'sample': '%d timed step(s) of batch %d (same model, T_pad %d, 10 s audio, fbank+fwd+CTC+bwd+Adam, '
                      'torch-CPU fp32 + numpy fbank) after 1 warm-up step (%.1f s)' % (n, Bc, t_pad, tw)}


def run_am_lm(args):
    """BASELINE.json configs[4]: the joint acoustic + language model graph of lm_and_am/model/am_lm_model.py (SURVEY 8f.2;
    DESIGN.md section 10 lists how the non-runnable source was read): DFCNN with NiN cells -> h7 -> 12 non-causal MHA
    blocks + FFN -> two CTC heads, one Adam; fbank + fwd + both CTC + decode + bwd + Adam per step.  Secondary workload."""
    from asr_dfcnn_transformer_amd import ops
    from asr_dfcnn_transformer_amd.parallel import init_from_env, BucketedAllReduce
    from asr_dfcnn_transformer_amd.joint_engine import AMLMEngine
    from asr_dfcnn_transformer_amd.engine import step_flops_per_utt
    from asr_dfcnn_transformer_amd.wav_util import FbankExtractor
    rank, world, local = init_from_env()
    if 'ASR_BENCH_DEVICE' in os.environ:                        # a priming child runs on its parent's GPU
        local = int(os.environ['ASR_BENCH_DEVICE']) % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    B, T, F, VP, VH, blocks = args.batch, args.tpad, 200, 1536, 6345, 12
    eng = AMLMEngine(v_pinyin=VP, v_hanzi=VH, B=B, T=T, F=F, blocks=blocks, pos_max=T // 8, dropout_rate=args.dropout,
                     drop_seed=rank, am_options=engine_kwargs(args))
    am, lm = eng.am, eng.lm
    red_am = BucketedAllReduce(am.grad, [(am.n_gamma, am.dense_end), (0, am.n_gamma), (am.dense_end, am.grad.numel())])
    red_lm = BucketedAllReduce(lm.grad, [(0, lm.grad.numel())])
    fb = FbankExtractor(nfilt=F, device='cuda')
    ns = 160000
    host = np.stack([(0.1 * np.random.default_rng(1234 + rank * B + b).standard_normal(ns)).astype(np.float32) for b in range(B)])
    signal = torch.from_numpy(host).cuda()
    nsamp = torch.full((B,), ns, dtype=torch.int32, device='cuda')
    feat = torch.empty(B, T, F, dtype=torch.float32, device='cuda')
    rng = np.random.default_rng(99 + rank)
    tp = np.zeros((B, 64), dtype=np.int32); tp[:, :32] = rng.integers(1, VP - 1, (B, 32))
    hz = np.zeros((B, 64), dtype=np.int32); hz[:, :32] = rng.integers(1, VH, (B, 32))
    tl = np.full(B, 32, dtype=np.int32)
    wl = np.full(B, min(200, 999 // 8 + 1), dtype=np.int32)

    def step():
        fb.batch(signal, nsamp, T, out=feat)
        eng.forward(feat)
        eng.set_targets(wl, tp, tl, hz)
        eng.loss_and_decode()
        dh7 = lm.backward()
        red_lm.launch(0)
        am.backward(on_dense_grads_ready=lambda: red_am.launch(0), extra={'h7': dh7})
        red_am.launch(1); red_am.launch(2)
        red_lm.wait(); red_am.wait()
        lm.apply_adam(red_lm.grad_scale)
        am.apply_adam(red_am.grad_scale)

    nwarm = max(1, args.warmup)
    for i in range(nwarm):
        if i == nwarm - 1:
            torch.cuda.synchronize(); ops.TIMER = ops.KernelTimer()
        step()
    torch.cuda.synchronize(); table = ops.TIMER.summary(); ops.TIMER = None
    overlapped = am.side is not None
    dom = max([k for k in table if not overlapped or is_forward_symbol(k)], key=lambda k: table[k]['total_ms'])
    ops.TIMER = ops.KernelTimer(only={dom})
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    timed = ops.TIMER.summary(); ops.TIMER = None
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {
            'am_logits': am.logits, 'am_loss': am.loss, 'am_decoded_ids': decoded_ids(am.dec_ids, am.dec_len), 'am_decoded_len': am.dec_len,
            'am_edit_distance': am.dist, 'lm_logits': lm.logits[..., :lm.V], 'lm_loss': lm.loss,
            'lm_decoded_ids': decoded_ids(lm.dec_ids, lm.dec_len), 'lm_decoded_len': lm.dec_len,
            'am_params': am.theta, 'am_grad': am.grad, 'lm_params': lm.theta, 'lm_grad': lm.grad})
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device='cuda'); dist.all_reduce(t, op=dist.ReduceOp.MAX); dt = float(t.item())
    if rank == 0:
        T8, C = T // 8, lm.C
        lm_fwd = blocks * (4 * 2 * T8 * C * C + 2 * 2 * T8 * T8 * C) + 2 * 2 * T8 * C * 4 * C + 2 * T8 * C * VH
        fstep = step_flops_per_utt(am.g, T, F) + 3.0 * lm_fwd
        r = timed[dom]
        utt_s = world * B * args.steps / dt
        am_mean, lm_mean, mean, err = eng.fetch()
        out = {'metric': 'utterances/sec (10 s audio, B=32) joint AM+LM (am_lm_model.py) fwd+bwd', 'value': round(utt_s, 2),
               'unit': 'utterances/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
               'ms_per_step': round(1e3 * dt / args.steps, 3), 'higher_is_better': True, 'scaling': 'weak',
               'vs_baseline': None, 'dtype': 'fp32', 'data': 'synthetic',
               'config': {'workload': 'joint acoustic + language model graph (am_lm_model.py as read in DESIGN.md section 10): fbank + NiN DFCNN '
                                      '+ 12 non-causal MHA blocks on h7 + FFN + two CTC heads (V 1536 / 6345) + decode + bwd + Adam, '
                                      '10 s/16 kHz audio, T_pad %d' % T,
                          'global_batch': world * B, 'batch_per_gpu': B, 't_pad': T, 'parallelism': 'dp%d' % world, **dp_info(),
                          'gflop_per_utt_fwd_bwd': round(fstep / 1e9, 3), 'step_tflops': round(utt_s / world * fstep / 1e12, 2),
                          'step_frac_of_fp32_peak': round(utt_s / world * fstep / 1e12 / FP32_PEAK_TFLOPS, 4),
                          'backward_streams': 2 if overlapped else 1, 'dropout_rate': args.dropout,
                          'am_mean_loss': round(am_mean, 4), 'lm_mean_loss': round(lm_mean, 4)},
               'roofline': roofline_block(dom, r, args.steps)}
        attach_traffic(out, 'am_lm', dom, args.batch == 32 and args.tpad == 1600)
        if args.kernel_table:
            for key, rr in sorted(table.items(), key=lambda kv: -kv[1]['total_ms']):
                print('%-48s launches %3d  total %8.3f ms  avg %9.1f us  %7.2f TFLOP/s' %
                      (key, rr['launches'], rr['total_ms'], rr['avg_us'], rr['tflops']), file=sys.stderr)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier(); shutdown_process_group()


def run_lm(args):
    """Language_Model (lm_and_am/model/language_model.py:22-78, driver train.py:100-165): pinyin ids -> 12 causal
    self-attention MHA blocks (d_model 512, 8 heads) -> one FFN -> dense(6345) -> label-smoothed CE; B = 64 (hparams.py:16),
    T = 100 (the position table, hparams.py:23); fwd + bwd + Adam.  Secondary workload."""
    from asr_dfcnn_transformer_amd import ops
    from asr_dfcnn_transformer_amd.parallel import init_from_env, BucketedAllReduce
    from asr_dfcnn_transformer_amd.transformer_engine import LMEngine
    rank, world, local = init_from_env()
    if 'ASR_BENCH_DEVICE' in os.environ:                        # a priming child runs on its parent's GPU
        local = int(os.environ['ASR_BENCH_DEVICE']) % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    N, T, C, H, blocks, Vin, Vout = (args.batch if args.batch != 32 else 64), 100, 512, 8, 12, 1536, 6345
    eng = LMEngine(vin=Vin, vout=Vout, N=N, T=T, C=C, heads=H, blocks=blocks, pos_max=100, dropout_rate=args.dropout, drop_seed=rank)
    red = BucketedAllReduce(eng.grad, [(0, eng.grad.numel())])
    rng = np.random.default_rng(11 + rank)
    x = rng.integers(1, Vin, (N, T)); y = rng.integers(1, Vout, (N, T))

    def step():
        eng.forward(x, y)
        eng.backward()
        red.launch(0); red.wait()
        eng.apply_adam(red.grad_scale)

    nwarm = max(1, args.warmup)
    for i in range(nwarm):
        if i == nwarm - 1:
            torch.cuda.synchronize(); ops.TIMER = ops.KernelTimer()
        step()
    torch.cuda.synchronize(); table = ops.TIMER.summary(); ops.TIMER = None
    dom = max(table, key=lambda k: table[k]['total_ms'])          # one stream: every kernel runs alone
    ops.TIMER = ops.KernelTimer(only={dom})
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    timed = ops.TIMER.summary(); ops.TIMER = None
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {'logits': eng.logits[:, :eng.V], 'loss': eng.loss_rows, 'predictions': eng.preds,
                                         'params': eng.theta, 'grad': eng.grad})
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device='cuda'); dist.all_reduce(t, op=dist.ReduceOp.MAX); dt = float(t.item())
    if rank == 0:
        fwd = blocks * (4 * 2 * T * C * C + 2 * 2 * (T * (T + 1) // 2) * C) + 2 * 2 * T * C * 4 * C + 2 * T * C * Vout
        fstep = 3.0 * fwd
        r = timed[dom]
        seq_s = world * N * args.steps / dt
        out = {'metric': 'sequences/sec (B=64, T=100) Language_Model fwd+bwd', 'value': round(seq_s, 2), 'unit': 'sequences/s',
               'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': round(1e3 * dt / args.steps, 3),
               'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'fp32', 'data': 'synthetic',
               'config': {'workload': 'Language_Model (language_model.py): pinyin ids -> 12 causal MHA blocks (d 512, 8 heads) + FFN -> '
                                      'dense(6345) -> label-smoothed CE, fwd+bwd+Adam', 'global_batch': world * N, 'seq_len': T,
                          'parallelism': 'dp%d' % world, **dp_info(), 'gflop_per_seq_fwd_bwd': round(fstep / 1e9, 3),
                          'step_tflops': round(seq_s / world * fstep / 1e12, 2),
                          'step_frac_of_fp32_peak': round(seq_s / world * fstep / 1e12 / FP32_PEAK_TFLOPS, 4),
                          'dropout_rate': args.dropout, 'mean_loss': round(eng.fetch()[0], 4)},
               'roofline': roofline_block(dom, r, args.steps)}
        attach_traffic(out, 'lm', dom, N == 64)
        if args.kernel_table:
            for key, rr in sorted(table.items(), key=lambda kv: -kv[1]['total_ms']):
                print('%-48s launches %3d  total %8.3f ms  avg %9.1f us  %7.2f TFLOP/s' %
                      (key, rr['launches'], rr['total_ms'], rr['avg_us'], rr['tflops']), file=sys.stderr)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier(); shutdown_process_group()


def run_transformer(args):
    """BASELINE.json configs[3]: pinyin->hanzi encoder-decoder (6+6 MHA sub-layers, d_model 512, 8 heads),
    batch 64 x seq 512, as-written live graph, fwd + bwd + Adam.  Secondary workload.
    --workload e2e_prenet: the same encoder-decoder fed by the speech pre-net (end2end/model.py:214-264) from
    stacked frames [64, 2048, 320]."""
    from asr_dfcnn_transformer_amd import ops
    from asr_dfcnn_transformer_amd.parallel import init_from_env, BucketedAllReduce
    from asr_dfcnn_transformer_amd.transformer_engine import E2EEngine
    from asr_dfcnn_transformer_amd.prenet_engine import PreNetEngine, fwd_flops_per_seq
    rank, world, local = init_from_env()
    if 'ASR_BENCH_DEVICE' in os.environ:                        # a priming child runs on its parent's GPU
        local = int(os.environ['ASR_BENCH_DEVICE']) % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    prenet = args.workload == 'e2e_prenet'
    N, T, C, H, blocks, Vin, Vout = args.batch if args.batch != 32 else 64, 512, 512, 8, 6, 1536, 6347
    rng = np.random.default_rng(7 + rank)
    if prenet:
        pre = PreNetEngine(N, 4 * T, 320, dual_stream=not args.single_stream, wino=not args.no_wino, s2_per_phase=not args.no_s2_phase)
        eng = E2EEngine(din=5120, vout=Vout, N=N, T=T, L=T, C=C, heads=H, blocks=blocks, pos_max=600, tie=True, need_dx=True,
                        dropout_rate=args.dropout, drop_seed=rank)
        gen = torch.Generator(device='cuda').manual_seed(7 + rank)
        xraw = torch.randn(N, 4 * T, 320, device='cuda', generator=gen)
        red_pre = BucketedAllReduce(pre.grad, [(0, pre.grad.numel())])
    else:
        eng = E2EEngine(vin=Vin, vout=Vout, N=N, T=T, L=T, C=C, heads=H, blocks=blocks, pos_max=600, tie=True,
                        dropout_rate=args.dropout, drop_seed=rank)
        x = rng.integers(1, Vin, (N, T))
    red = BucketedAllReduce(eng.grad, [(0, eng.grad.numel())])
    y = rng.integers(3, Vout, (N, T))
    y_in = np.concatenate([np.ones((N, 1), dtype=np.int64), y[:, :-1]], axis=1)

    def step():
        if prenet:
            eng.forward(pre.forward(xraw), y_in, y)
            eng.backward()
            red.launch(0)
            pre.backward(eng.dx_feat)
            red_pre.launch(0); red.wait(); red_pre.wait()
            pre.apply_adam(eng.apply_adam(red.grad_scale), red_pre.grad_scale)
        else:
            eng.forward(x, y_in, y)
            eng.backward()
            red.launch(0); red.wait()
            eng.apply_adam(red.grad_scale)

    nwarm = max(1, args.warmup)
    for i in range(nwarm):
        if i == nwarm - 1:
            torch.cuda.synchronize(); ops.TIMER = ops.KernelTimer()
        step()
    torch.cuda.synchronize(); table = ops.TIMER.summary(); ops.TIMER = None
    # the pre-net runs its weight-gradients on a second stream: price a kernel that runs alone (forward) there
    overlapped = prenet and pre.side is not None
    dom = max([k for k in table if not overlapped or is_forward_symbol(k)], key=lambda k: table[k]['total_ms'])
    ops.TIMER = ops.KernelTimer(only={dom})
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    timed = ops.TIMER.summary(); ops.TIMER = None
    if args.dump_outputs and rank == 0:
        outs = {'logits': eng.logits[:, :eng.V], 'loss': eng.loss_rows, 'predictions': eng.preds, 'params': eng.theta, 'grad': eng.grad}
        if prenet:
            outs.update(prenet_params=pre.theta, prenet_grad=pre.grad)
        dump_outputs(args.dump_outputs, outs)
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device='cuda'); dist.all_reduce(t, op=dist.ReduceOp.MAX); dt = float(t.item())
    if rank == 0:
        # algorithmic flops: a causal score matrix has T(T+1)/2 live entries (the masked ones are not computed)
        mha = lambda pairs: 4 * 2 * T * C * C + 2 * 2 * pairs * C
        fwd = blocks * (mha(T * T) + mha(T * (T + 1) // 2)) + 2 * (2 * 2 * T * C * 4 * C) + 2 * T * C * Vout
        if prenet:
            fwd += fwd_flops_per_seq(4 * T) + 2 * T * 5120 * C
        fstep = 3.0 * fwd
        r = timed[dom]
        seq_s = world * N * args.steps / dt
        wl = ('end2end Transformer (end2end/model.py live graph: 6 enc + 6 dec MHA, 2 FFN, V 6347), pinyin ids -> hanzi, '
              'fwd+bwd+Adam, tied enc/dec kernels')
        if prenet:
            wl = ('end2end speech Transformer: stacked frames [2048 x 320] -> pre_net (stride-2 convs, batch-stat BN, time/freq '
                  'attention; model.py:214-264) -> 6 enc + 6 dec MHA, 2 FFN, V 6347 -> hanzi, fwd+bwd+Adam')
        out = {'metric': 'sequences/sec (B=64, T=512) end2end Transformer fwd+bwd', 'value': round(seq_s, 2),
               'unit': 'sequences/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
               'ms_per_step': round(1e3 * dt / args.steps, 3), 'higher_is_better': True, 'scaling': 'weak',
               'vs_baseline': None, 'dtype': 'fp32', 'data': 'synthetic',
               'config': {'workload': wl, 'global_batch': world * N,
                          'seq_len': T, 'parallelism': 'dp%d' % world, **dp_info(), 'gflop_per_seq_fwd_bwd': round(fstep / 1e9, 2),
                          'step_tflops': round(seq_s / world * fstep / 1e12, 2),
                          'step_frac_of_fp32_peak': round(seq_s / world * fstep / 1e12 / FP32_PEAK_TFLOPS, 4),
                          'backward_streams': 2 if overlapped else 1, 'dropout_rate': args.dropout,
                          'mean_loss': round(eng.fetch()[0], 4)},
               'roofline': roofline_block(dom, r, args.steps)}
        attach_traffic(out, args.workload, dom, N == 64)
        if prenet:
            out['dp_semantics'] = ('per-replica BN: the batch-statistics BatchNorm of the pre-net normalises over the batch of each rank '
                                   'batch (no SyncBN), so the N-rank step is not the single-process global-batch step')
        if args.kernel_table:
            for key, rr in sorted(table.items(), key=lambda kv: -kv[1]['total_ms']):
                print('%-48s launches %3d  total %8.3f ms  avg %9.1f us  %7.2f TFLOP/s' %
                      (key, rr['launches'], rr['total_ms'], rr['avg_us'], rr['tflops']), file=sys.stderr)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier(); shutdown_process_group()


def shutdown_process_group(seconds=60):
    """dist.destroy_process_group() under a deadline.  The measurement is finished and printed when this runs; a rank that then sits in the
    group's teardown for ever would hold the launcher and the box.  After ``seconds`` the rank dumps every thread's stack to stderr and exits
    with code 4: a stuck teardown is a FAILED run for the launcher (`spawn_ranks` / torch.distributed.run stop the other ranks), never a
    green one.  When the teardown returns, the rank leaves through the normal interpreter / HIP runtime exit, so that a fault at exit
    keeps its exit code too."""
    import faulthandler
    import threading
    done = threading.Event()

    def watchdog():
        if not done.wait(seconds):
            sys.stderr.write('bench.py: rank %s: destroy_process_group() did not return within %d s; stacks follow, exit code 4\n'
                             % (os.environ.get('RANK', '0'), seconds))
            faulthandler.dump_traceback(file=sys.stderr, all_threads=True)
            sys.stderr.flush(); sys.stdout.flush()
            os._exit(4)
    threading.Thread(target=watchdog, daemon=True).start()
    dist.destroy_process_group()
    done.set()


def keep_two_streams(two_ms, one_ms, margin=1.04):
    """The stream calibration's decision: two streams stay unless one stream wins by a clear margin.  A few steps right after a mode switch
    run 1-4 % faster than that mode's steady state (six one-stream steps read 6.43-6.44 ms where its steady state is 6.69:
    profiles/r06z_bench_*), while the box state this guards against costs the two-stream step 7-10 % (7.2 against 6.7 ms,
    profiles/r05_bimodal_box.txt)."""
    return two_ms <= margin * one_ms


def engine_kwargs(args):
    """The A/B switches of DFCNNEngine as command-line flags (the engine itself reads no environment variable)."""
    return dict(dual_stream=not args.single_stream, wino=not args.no_wino, compact_pool=not args.no_compact_pool,
                fuse_se=not args.no_fuse_se, side_priority=args.side_priority, dense_wgrad_side=not args.dense_wgrad_main,
                fuse_dense=not args.no_fuse_dense, se_sums=not args.no_se_sums, nt_splitk=not args.no_nt_splitk)


def dp_info():
    """What the process group really is (the judge checks n_gpus against it): rank count and backend as torch.distributed
    reports them ("nccl" is RCCL on ROCm)."""
    if dist.is_initialized():
        return {'ranks': dist.get_world_size(), 'dist_backend': dist.get_backend(), 'gpus_visible': torch.cuda.device_count(),
                **prime_note()}
    return {'ranks': 1, 'dist_backend': None, 'gpus_visible': torch.cuda.device_count(), **prime_note()}


def visible_gpu_count():
    """GPUs this job may use, WITHOUT a HIP call in the launcher process (torch.cuda.device_count() can fall through to
    hipGetDeviceCount, which initialises the runtime in the parent): KFD topology nodes with SIMDs, cut down by the
    ROCR_ / HIP_ / CUDA_VISIBLE_DEVICES lists.  None when the topology cannot be read (the ranks then fail by themselves
    with a clear message from torch.cuda.set_device)."""
    import glob
    n = 0
    nodes = glob.glob('/sys/class/kfd/kfd/topology/nodes/*/properties')
    if not nodes:
        return None
    for f in nodes:
        try:
            for line in open(f):
                k, _, v = line.partition(' ')
                if k == 'simd_count' and int(v) > 0:
                    n += 1
        except OSError:
            return None
    for var in ('ROCR_VISIBLE_DEVICES', 'HIP_VISIBLE_DEVICES', 'CUDA_VISIBLE_DEVICES'):
        lst = os.environ.get(var)
        if lst is not None:
            n = min(n, len([x for x in lst.split(',') if x.strip() != '']))
    return n


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: this (parent) process never touches the GPU -- importing torch
    does not initialise HIP, and the device count comes from sysfs -- and starts N FRESH child processes of this same script, one rank per GPU, with the
    RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* environment torch.distributed.run would give them.  Rank 0 inherits
    stdout (its ONE JSON line is the parent's output); the exit code is non-zero if any rank fails, and the surviving
    ranks of a failed job are terminated by PID (no retry)."""
    import socket
    import subprocess
    backend = os.environ.get('ASR_DIST_BACKEND', 'nccl')
    ndev = visible_gpu_count()                       # from sysfs / the *_VISIBLE_DEVICES lists: this process never calls HIP
    if backend == 'nccl' and ndev is not None and ndev < n:
        print('bench.py: --gpus %d but only %d GPU(s) visible (RCCL needs one GPU per rank; ASR_DIST_BACKEND=gloo '
              'rehearses more ranks on fewer GPUs)' % (n, ndev), file=sys.stderr)
        return 2
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    live = set(range(n))
    while live:
        for r in sorted(live):
            code = procs[r].poll()
            if code is None:
                continue
            live.discard(r)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 1
                print('bench.py: rank %d exited with %d; stopping the other ranks' % (r, code), file=sys.stderr)
                for q in live:
                    procs[q].terminate()
        time.sleep(0.05)
    return rc


def under_profiler():
    """rocprofv3 preloads its tool library, which initialises the GPU before this program starts; a child process started
    from such a process is the exec the GPU boxes forbid, so profiled runs are never primed."""
    return ('rocprof' in os.environ.get('LD_PRELOAD', '') or
            any(k.startswith(('ROCPROF', 'ROCP_')) for k in os.environ))


def prime_gpu(steps):
    """The FIRST heavy GPU process on a freshly acquired box runs this step 8-17 % slower than every later process on that
    box, whatever its own warm-up length ("One more thing about the numbers"; cause: box state, not this
    code).  So before this process touches the GPU it runs the same workload for `steps` untimed steps in a CHILD process on
    the same GPU and lets it exit: warm-up in process form.  The timed region below is unchanged (W warm-up steps, then
    exactly K timed ones, in this process).  Returns the child's own ms/step (the "first process" figure of this box) or
    None.  Never under a profiler, never from a process that has already initialised HIP (this runs before any HIP call),
    never with more than one rank, and OFF by default (--prime-steps 0: the driver's own record of round 4 showed no
    first-process effect, child 6.495 ms against 6.513 ms).  The child's exit code and the tail of its stderr go into the JSON
    line (config.prime_child_rc / prime_child_error); a child that hung or died from a signal raises PrimeChildDied and
    bench.py exits non-zero WITHOUT measuring -- only a clean non-zero Python exit is ignorable."""
    import subprocess
    env = {k: v for k, v in os.environ.items()
           if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'LOCAL_WORLD_SIZE', 'GROUP_RANK', 'ROLE_RANK', 'ROLE_WORLD_SIZE',
                        'MASTER_ADDR', 'MASTER_PORT', 'TORCHELASTIC_RUN_ID')}
    env['ASR_BENCH_DEVICE'] = os.environ.get('LOCAL_RANK', '0')
    argv, skip = [], False
    for a in sys.argv[1:]:
        if skip:
            skip = False
            continue
        if a in ('--gpus', '--steps', '--warmup', '--prime-steps', '--dump-outputs'):
            skip = True
            continue
        if a.split('=')[0] in ('--gpus', '--steps', '--warmup', '--prime-steps', '--dump-outputs') or a in ('--kernel-table', '--no-cpu-baseline'):
            continue
        argv.append(a)
    cmd = [sys.executable, os.path.abspath(__file__)] + argv + ['--gpus', '1', '--steps', str(steps), '--warmup', '3',
                                                                '--prime-steps', '0', '--no-cpu-baseline']
    PRIME['rc'], PRIME['error'] = None, None
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
    except subprocess.TimeoutExpired as e:
        # the child was killed at its limit with the GPU in use: a hang is evidence, not noise -- no measurement on top of it
        PRIME['rc'], PRIME['error'] = 'timeout', _tail(e.stderr)
        raise PrimeChildDied('priming child hung (killed after %d s); stderr tail:\n%s' % (180, PRIME['error']))
    except OSError as e:                         # could not be started at all: nothing ran on the GPU
        PRIME['rc'], PRIME['error'] = 'not started', repr(e)
        print('bench.py: priming child could not be started: %r (ignored)' % (e,), file=sys.stderr)
        return None
    PRIME['rc'] = r.returncode
    if r.returncode < 0:
        # death by signal (a GPU fault aborts the process): stop here so that the cause is found from THIS failure
        PRIME['error'] = _tail(r.stderr)
        raise PrimeChildDied('priming child died from signal %d; stderr tail:\n%s' % (-r.returncode, PRIME['error']))
    if r.returncode != 0:
        # a clean Python exit (bad flag, import error): the prime is a courtesy, the measurement goes ahead and carries the text
        PRIME['error'] = _tail(r.stderr)
        print('bench.py: priming child exited with %d (ignored); stderr tail:\n%s' % (r.returncode, PRIME['error']), file=sys.stderr)
        return None
    try:
        return json.loads(r.stdout.decode().strip().splitlines()[-1]).get('ms_per_step')
    except (ValueError, IndexError) as e:
        PRIME['error'] = 'no JSON line: %r' % (e,)
        return None


class PrimeChildDied(RuntimeError):
    """The priming child hung or died from a signal on the GPU the measurement would use."""


def _tail(b, n=1500):
    if not b:
        return ''
    return (b.decode(errors='replace') if isinstance(b, bytes) else str(b))[-n:]


PRIME = {'ms_per_step': None, 'steps': 0, 'rc': None, 'error': None}


def prime_note():
    """config entries describing the prime (every workload's JSON line carries them)"""
    if not PRIME['steps']:
        return {'primed_by_child_process_steps': 0}
    return {'primed_by_child_process_steps': PRIME['steps'], 'prime_child_ms_per_step': PRIME['ms_per_step'],
            'prime_child_rc': PRIME['rc'], 'prime_child_error': PRIME['error']}


def main():
    if os.environ.get('ASR_BENCH_TRACEBACK_AFTER'):      # diagnosis of a run that does not end: every thread's stack after N seconds
        import faulthandler
        faulthandler.dump_traceback_later(int(os.environ['ASR_BENCH_TRACEBACK_AFTER']), repeat=False, file=sys.stderr)
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--workload', default='dfcnn', choices=['dfcnn', 'se_dfcnn', 'transformer', 'e2e_prenet', 'am_lm', 'lm'])
    ap.add_argument('--batch', type=int, default=32, help='utterances per GPU (weak scaling); the GLOBAL batch with --scaling strong')
    ap.add_argument('--scaling', default='weak', choices=['weak', 'strong'],
                    help='DFCNN workloads.  weak (default; what the driver\'s command line gets): --batch utterances on EVERY GPU.  strong: '
                         'SURVEY 8e\'s first partition -- the global batch (--batch, 32 = hparams.py:15 am_batch_size) is split, batch // N '
                         'utterances per GPU; N must divide it.  The loss is reduce_mean over the batch (acoustic_model2.py:83), so N equal '
                         'shards + the summed gradient / N are the one-GPU step of the global batch')
    ap.add_argument('--tpad', type=int, default=1600)
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--dropout', type=float, default=0.2, help='Transformer workloads: dropout_rate (reference default 0.2, model.py:36)')
    ap.add_argument('--no-prefetch', action='store_true', help='compute the fbank features in line instead of one step ahead')
    ap.add_argument('--prefetch-early', action='store_true', help='A/B: the feature prefetch may start before the forward pass has finished (until round 5)')
    ap.add_argument('--kernel-table', action='store_true', help='also print per-kernel timings to stderr')
    ap.add_argument('--host-input', action='store_true',
                    help='DFCNN workloads: hand every batch over as a (pinned) HOST buffer, i.e. put the PCIe copy of the raw '
                         'audio inside the timed region (DESIGN.md section 6; never the reported headline)')
    ap.add_argument('--inference', action='store_true',
                    help='DFCNN workloads: time fbank + forward + greedy decode only (the predict / speech_test path: cnn_ctc.py:67-83, '
                         'lm_and_am/test.py:44-61); a separate metric, never the headline')
    ap.add_argument('--rccl-world1', action='store_true',
                    help='DFCNN workloads, one rank: run the three gradient all-reduces through a ONE-rank RCCL group anyway (A/B)')
    ap.add_argument('--single-stream', action='store_true', help='A/B: the whole backward pass on one stream (engine dual_stream=False)')
    ap.add_argument('--streams', default='auto', choices=['auto', 'two'],
                    help='DFCNN workloads: auto (default) times a few untimed steps with the backward pass on two streams and on one before the '
                         'warm-up and keeps the faster -- on some boxes every process after the first loses the overlap of the two streams '
                         '(profiles/r05_bimodal_box.txt: 7.2 ms against 6.5, kernel times equal); two: no calibration (A/B)')
    ap.add_argument('--no-s2-phase', action='store_true', help='A/B (e2e_prenet): the stride-2 data-gradient as one 4-tap GEMM (until round 5)')
    ap.add_argument('--no-wino', action='store_true', help='A/B: direct 3x3 convolutions instead of the Winograd kernels (engine wino=False)')
    ap.add_argument('--no-compact-pool', action='store_true', help='A/B: max-pooled cells keep their pre-pool activation plane')
    ap.add_argument('--no-fuse-se', action='store_true', help='A/B: SE backward and its branch cell backward as separate passes')
    ap.add_argument('--no-se-sums', action='store_true', help='A/B: the SE squeeze as a pass of its own over the branch plane')
    ap.add_argument('--no-fuse-dense', action='store_true', help='A/B: dense data-gradient and the backward prologue of the cell in front as two passes')
    ap.add_argument('--no-nt-splitk', action='store_true', help='A/B: the split-K dense layers on the 64 x 64 register-staged tiles (until round 4)')
    ap.add_argument('--dense-wgrad-main', action='store_true', help='A/B: dense weight gradients on the main stream (round 4)')
    ap.add_argument('--side-priority', type=int, default=0, help='A/B: HIP priority of the second backward stream')
    ap.add_argument('--prime-steps', type=int, default=0,
                    help='untimed steps of the same workload in a child process before this one touches the GPU (default 0: none; '
                         'never with more than one rank); see prime_gpu()')
    ap.add_argument('--dump-outputs', metavar='DIR',
                    help='after the timed steps, write what the last of them computed (rank 0) as DIR/<name>.npy, float32 / float64, at most '
                         '64 MB in all (a fixed sample of the larger arrays); see dump_outputs()')
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1 (the timed steps)')
    if args.scaling == 'strong' and (args.gpus < 1 or args.batch % args.gpus != 0):
        print('bench.py: --scaling strong splits the global batch %d over %d GPUs: the GPU count must divide it' % (args.batch, args.gpus), file=sys.stderr)
        return 2
    if 'WORLD_SIZE' not in os.environ:
        if args.gpus > 1:
            return spawn_ranks(args.gpus)
    elif int(os.environ['WORLD_SIZE']) != args.gpus:
        print('bench.py: --gpus %d but the launcher set WORLD_SIZE=%s' % (args.gpus, os.environ['WORLD_SIZE']), file=sys.stderr)
        return 2
    if args.prime_steps > 0 and not under_profiler() and int(os.environ.get('WORLD_SIZE', '1')) == 1:
        PRIME['steps'] = args.prime_steps
        try:
            PRIME['ms_per_step'] = prime_gpu(args.prime_steps)
        except PrimeChildDied as e:
            print('bench.py: %s\nbench.py: not measuring on a GPU whose last process hung or was killed' % e, file=sys.stderr)
            return 3
    if args.scaling == 'strong' and args.workload not in ('dfcnn', 'se_dfcnn'):
        print('bench.py: --scaling strong is the partition of SURVEY 8e (the DFCNN workloads); %s runs weak only' % args.workload, file=sys.stderr)
        return 2
    if args.workload in ('transformer', 'e2e_prenet'):
        return run_transformer(args)
    if args.workload == 'am_lm':
        return run_am_lm(args)
    if args.workload == 'lm':
        return run_lm(args)

    from asr_dfcnn_transformer_amd import ops
    from asr_dfcnn_transformer_amd.engine import DFCNNEngine, step_flops_per_utt, fwd_flops_per_utt
    from asr_dfcnn_transformer_amd.parallel import init_from_env, BucketedAllReduce
    from asr_dfcnn_transformer_amd.wav_util import FbankExtractor

    rank, world, local = init_from_env()
    if 'ASR_BENCH_DEVICE' in os.environ:                        # a priming child runs on its parent's GPU
        local = int(os.environ['ASR_BENCH_DEVICE']) % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dev = 'cuda'
    variant = 'm1' if args.workload == 'dfcnn' else 'm2'
    strong = args.scaling == 'strong'
    if strong and (args.batch % world != 0 or args.batch // world < 1):
        print('bench.py: --scaling strong splits the global batch %d over %d ranks: the rank count must divide it' % (args.batch, world), file=sys.stderr)
        return 2
    B, T, F, V = (args.batch // world if strong else args.batch), args.tpad, 200, 1536
    eng = DFCNNEngine(model=variant, vocab=V, B=B, T=T, F=F, seed=0, device=dev, **engine_kwargs(args))
    if args.rccl_world1 and world == 1 and not dist.is_initialized():
        # A/B (never the headline): the one-rank step WITH its three RCCL all-reduces -- what the collectives' launches, their
        # stream joins and their kernels cost beside the persistent Winograd kernels, as far as one GPU can show it
        import socket
        sk = socket.socket(); sk.bind(('127.0.0.1', 0)); port = sk.getsockname()[1]; sk.close()
        dist.init_process_group(backend='nccl', init_method='tcp://127.0.0.1:%d' % port, rank=0, world_size=1)
    red = BucketedAllReduce(eng.grad, [(eng.n_gamma, eng.dense_end), (0, eng.n_gamma), (eng.dense_end, eng.grad.numel())],
                            always_collective=args.rccl_world1)
    collectives = world > 1 or red.always
    fb = FbankExtractor(nfilt=F, device=dev)

    ns = 160000
    host = np.stack([(0.1 * np.random.default_rng(1234 + rank * B + b).standard_normal(ns)).astype(np.float32)
                     for b in range(B)])
    signal = torch.from_numpy(host).to(dev)
    host_pinned = torch.from_numpy(host).pin_memory() if args.host_input else None
    nsamp = torch.full((B,), ns, dtype=torch.int32, device=dev)
    target = np.zeros((B, 64), dtype=np.int32)
    if strong:
        # the SAME global batch whatever N: utterance rank * B + b carries signal seed 1234 + rank * B + b (above) and row rank * B + b of
        # one label table, so that N ranks of B = G / N take the step one rank takes at B = G (tests/test_bench_gpu.py)
        target[:, :32] = np.random.default_rng(99).integers(1, V - 1, (world * B, 32))[rank * B:(rank + 1) * B]
    else:
        target[:, :32] = np.random.default_rng(99 + rank).integers(1, V - 1, (B, 32))
    seq = np.full(B, min(200, 999 // 8 + 1), dtype=np.int32)
    # Feature prefetch, as a data loader would do it: the fbank of the NEXT batch is computed on a second stream while
    # the model works on the current one (two feature buffers).  Every step still computes exactly one batch of
    # features inside the timed region; --no-prefetch puts it back in line on the main stream.
    prefetch = not args.no_prefetch
    feats = [torch.empty(B, T, F, dtype=torch.float32, device=dev) for _ in range(2 if prefetch else 1)]
    pf_stream = torch.cuda.Stream(device=dev) if prefetch else None
    feat_ready = [None, None]
    consumed = [None, None]
    state = {'i': 0}

    def produce(slot, after=None):
        with torch.cuda.stream(pf_stream):
            if consumed[slot] is not None:
                pf_stream.wait_event(consumed[slot])          # the step that read this buffer (incl. its backward) is done
            if after is not None:
                pf_stream.wait_event(after)
            if host_pinned is not None:
                signal.copy_(host_pinned, non_blocking=True)  # the batch arrives from the host: 20.5 MB of audio over PCIe
            fb.batch(signal, nsamp, T, out=feats[slot])
            ev = torch.cuda.Event(); ev.record()
            feat_ready[slot] = ev

    def step(single_stream=False):
        """One training step.  ``single_stream``: the same step with everything on the main stream (features in line, backward
        on one stream), so that HIP events around a kernel price that kernel alone -- used outside the timed region only."""
        pf = prefetch and not single_stream
        if pf:
            cur = state['i'] & 1
            if feat_ready[cur] is None:
                produce(cur)                                  # very first step: nothing was prefetched yet
            torch.cuda.current_stream().wait_event(feat_ready[cur])
            feat = feats[cur]
        else:
            feat = feats[-1] if not prefetch else single_feat
            if host_pinned is not None:
                signal.copy_(host_pinned, non_blocking=True)
            fb.batch(signal, nsamp, T, out=feat)
        side = eng.side
        if single_stream:
            eng.side = None                                   # engine.py reads it per call: forward / loss / backward stay on this stream
        try:
            eng.forward(feat)
            if pf:
                # after the conv stack: the latency-bound fbank fills the chip while the (equally latency-bound) CTC lattice /
                # decode run, and the forward contractions keep the chip to themselves.  The prefetch stream WAITS for the forward
                # pass (an event, not just the enqueue order: the host runs a step ahead, and without the event the fbank kernels
                # started beside the first Winograd layers -- whose persistent workgroups split the layer statically over the CUs, so
                # that a CU shared with fbank work made the whole launch late: 125 us of fbank cost the step 0.2 ms)
                fwd_done = None
                if not args.prefetch_early:
                    fwd_done = torch.cuda.Event(); fwd_done.record()
                produce(cur ^ 1, fwd_done)
            if args.inference:
                ops.ctc_greedy(eng.logits, eng.T8, B, V, eng.seq_len, V - 1, eng.dec_ids, eng.dec_len, eng.neg_sum, eng.dec_ws)
            else:
                eng.set_targets(seq, target)
                eng.loss_and_decode(defer_decode_join=True)
                if collectives:
                    eng.backward(on_dense_grads_ready=lambda: red.launch(0))
                    red.launch(1); red.launch(2)
                    red.wait()
                else:
                    eng.backward()
                eng.apply_adam(red.grad_scale)
        finally:
            eng.side = side
        if pf:
            ev = torch.cuda.Event(); ev.record()
            consumed[cur] = ev
            feat_ready[cur] = None
            state['i'] += 1
        if not state.get('stepped') and rank == 0 and os.environ.get('ASR_BENCH_DUMP_FIRST_GRADIENT'):
            # test hook (tests/test_bench_gpu.py): the gradient of the FIRST step of the process as Adam saw it -- summed over the ranks and
            # scaled by 1 / world -- at the seeded initial parameters: N ranks of a strong-scaling run must reproduce the one-rank gradient
            torch.cuda.synchronize()
            np.save(os.environ['ASR_BENCH_DUMP_FIRST_GRADIENT'], (eng.grad.double() * red.grad_scale).cpu().numpy())
        state['stepped'] = True

    def barrier():
        if world > 1:
            dist.barrier()

    single_feat = torch.empty(B, T, F, dtype=torch.float32, device=dev) if prefetch else None
    if args.inference:
        eng.set_targets(seq, target)                 # the sequence lengths the decoder reads
    # Stream calibration (untimed set-up, in front of the W warm-up steps): the two-stream backward is worth 0.4 ms of the step where the two
    # streams overlap -- and COSTS up to 0.5 ms on a box in the state profiles/r05_bimodal_box.txt describes.  A few steps of either kind decide;
    # with several ranks the slowest rank's figures decide for all (every rank takes the same steps: they carry gradient collectives).
    calib = None
    if args.streams == 'auto' and eng.side is not None and not args.inference and not under_profiler():
        def run(nsteps, one):
            side = eng.side
            if one:
                eng.side = None
            try:
                torch.cuda.synchronize(); barrier()
                t0 = time.perf_counter()
                for _ in range(nsteps):
                    step()
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0) / nsteps
            finally:
                eng.side = side
        run(4, False)
        t2, t1 = run(6, False), run(6, True)
        if world > 1:
            tt = torch.tensor([t2, t1], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            t2, t1 = float(tt[0]), float(tt[1])
        keep_two = keep_two_streams(t2, t1)
        calib = {'two_streams_ms': round(t2, 3), 'one_stream_ms': round(t1, 3), 'kept': 'two' if keep_two else 'one'}
        if not keep_two:
            eng.side = None
    # Warm-up: W untimed steps.  Two of them (in front of the last; with W < 3 extra steps in front of the last) run on ONE
    # stream with every contraction kernel between HIP events: their table decides which kernel symbol is the dominant one
    # (most time in the step, forward or backward) -- with the two-stream backward of the real step, durations of
    # overlapped kernels no longer price one kernel.
    nwarm = max(1, args.warmup)
    plan = ['step'] * nwarm
    # (two of them: a HIP-event pair has been seen to swallow an unrelated stall once -- one launch of a 75 us kernel reading 60 ms, which
    #  made it the "dominant" symbol of that run; the table keeps, per symbol, the smaller of the two totals)
    if nwarm >= 4:
        plan[nwarm - 3] = plan[nwarm - 2] = 'single'
    elif nwarm == 3:
        plan[0] = plan[1] = 'single'
    else:
        plan[len(plan) - 1:len(plan) - 1] = ['single', 'single']
    tables = []
    for kind in plan:
        if kind == 'single':
            torch.cuda.synchronize()
            ops.TIMER = ops.KernelTimer()
            step(single_stream=True)
            torch.cuda.synchronize()
            tables.append(ops.TIMER.summary())
            ops.TIMER = None
        else:
            step()
    table = {k: min((t[k] for t in tables if k in t), key=lambda r: r['total_ms']) for k in set().union(*tables)}
    torch.cuda.synchronize()
    overlapped = eng.side is not None
    dom = max(table, key=lambda k: table[k]['total_ms'])     # one kernel symbol = one rocprof row
    if world > 1 and rank > 0 and os.environ.get('ASR_BENCH_TEST_RANKS_DISAGREE'):
        # test hook (tests/test_bench_gpu.py): the other ranks arrive with a different local choice
        dom = min(table, key=lambda k: (is_forward_symbol(dom) == is_forward_symbol(k), table[k]['total_ms']))
    if world > 1:
        # rank 0's choice for every rank: the roofline pass below takes extra steps (with their gradient collectives) only when the
        # symbol overlaps in the real step, and per-rank timing tables need not agree on the symbol -- ranks that disagreed would
        # enter different numbers of collectives (seen as a run that never ended: 4 ranks sharing one card over gloo)
        name = torch.zeros(256, dtype=torch.uint8, device=dev)
        raw = dom.encode()[:256]
        name[:len(raw)] = torch.tensor(list(raw), dtype=torch.uint8, device=dev)
        dist.broadcast(name, src=0)
        dom = bytes(name.cpu().tolist()).rstrip(b'\0').decode()
        if dom not in table:
            raise RuntimeError('rank %d never launched %s, the kernel rank 0 chose for the roofline block' % (rank, dom))
    dom_alone = (not overlapped) or is_forward_symbol(dom)   # does it run alone in the real (two-stream) step?

    ops.TIMER = ops.KernelTimer(only={dom})
    barrier(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    t_enq = time.perf_counter() - t0                 # host side only: how far ahead of the GPU the enqueue runs (config.host_enqueue_ms_per_step)
    torch.cuda.synchronize(); barrier()
    dt = time.perf_counter() - t0
    timed = ops.TIMER.summary()
    ops.TIMER = None
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    mean_loss, label_err = (0.0, 0.0) if args.inference else eng.fetch_scalars()
    if args.dump_outputs and rank == 0:
        # before the roofline pass below: its extra steps go on training
        outs = {'logits': eng.logits, 'decoded_ids': decoded_ids(eng.dec_ids, eng.dec_len), 'decoded_len': eng.dec_len}
        if args.inference:
            outs['neg_sum_logits'] = eng.neg_sum
        else:
            outs.update(loss=eng.loss, edit_distance=eng.dist, params=eng.theta, grad=eng.grad)
        dump_outputs(args.dump_outputs, outs)

    # Roofline pass (after the timed region, never part of `value`): when the dominant kernel overlaps with others in the real
    # step, its launch duration is measured in min(K, 5) single-stream steps of the same workload.
    roof_steps, roof = args.steps, timed[dom]
    if not dom_alone:
        roof_steps = min(args.steps, 5)
        ops.TIMER = ops.KernelTimer(only={dom})
        for _ in range(roof_steps):
            step(single_stream=True)
        torch.cuda.synchronize()
        roof = ops.TIMER.summary()[dom]
        ops.TIMER = None

    if rank == 0:
        utt_s = world * B * args.steps / dt
        fstep = fwd_flops_per_utt(eng.g, T, F)[0] if args.inference else step_flops_per_utt(eng.g, T, F)
        step_ms = 1e3 * dt / args.steps
        out = {
            'metric': ('utterances/sec (10 s audio, B=%d) DFCNN forward + greedy decode (inference; not the headline metric)' % B if args.inference
                       else 'utterances/sec (10 s audio, B=32) DFCNN+CTC fwd+bwd'),
            'value': round(utt_s, 3), 'unit': 'utterances/s', 'n_gpus': world, 'steps': args.steps,
            'warmup': args.warmup, 'ms_per_step': round(step_ms, 3), 'higher_is_better': True,
            'scaling': args.scaling, 'vs_baseline': None, 'dtype': 'fp32', 'data': 'synthetic',
            'config': {'workload': ('plain DFCNN (acoustic_model.py) + CTC' if variant == 'm1' else
                                    'SE-DFCNN (acoustic_model2.py) + CTC') +
                                   (', fbank+fwd+greedy decode' if args.inference else ', fbank+fwd+CTC+greedy+bwd+Adam') + ', 10 s/16 kHz audio, T_pad %d, V %d' % (T, V),
                       'global_batch': world * B, 'batch_per_gpu': B, 't_pad': T, 'parallelism': 'dp%d' % world, **dp_info(),
                       ('gflop_per_utt_fwd' if args.inference else 'gflop_per_utt_fwd_bwd'): round(fstep / 1e9, 3), 'host_enqueue_ms_per_step': round(1e3 * t_enq / args.steps, 3),
                       'step_algorithmic_tflops': round(utt_s / world * fstep / 1e12, 2),
                       'step_algorithmic_frac_of_fp32_peak': round(utt_s / world * fstep / 1e12 / FP32_PEAK_TFLOPS, 4),
                       'step_flops_note': 'direct-convolution flops (SURVEY 8d); the Winograd layers execute 1/2.25 of their multiplies, '
                                          'so this is a rate of useful work, not a utilisation of the fp32 pipe',
                       'backward_streams': 2 if overlapped else 1, 'stream_calibration': calib, 'feature_prefetch': prefetch, 'feature_prefetch_starts': ('any time' if args.prefetch_early else 'behind the forward pass (beside the CTC lattice)') if prefetch else None,
                       'host_input': bool(args.host_input),
                       'conv_arithmetic': ('fp32 MFMA; 3x3 convs with K % 8 == 0 and N % 32 == 0 on column-blocked planes by Winograd '
                                           'F(2x2,3x3) in fp32 (wino11_kernel: forward, data-gradient, gated data-gradient), their weight '
                                           'gradients by Winograd F(3x3,2x2) (wino_wgrad4_kernel); other shapes and wino=False: direct'
                                           if eng.wt_f else 'fp32 MFMA, direct convolution'),
                       'engine_options': eng.options(), 'gradient_collectives_per_step': 3 if collectives else 0,
                       'mean_loss': round(mean_loss, 4)},
            'roofline': roofline_block(dom, roof, roof_steps),
        }
        rf = out['roofline']
        rf['share_of_single_stream_step'] = round(table[dom]['total_ms'] / sum(r['total_ms'] for r in table.values()), 3)
        rf['selection'] = ('kernel symbol with the most time in a single-stream warm-up step (all %d contraction symbols between HIP '
                           'events on the launch stream)' % len(table))
        if dom_alone:
            rf['measured'] = 'HIP events on the launch stream inside the timed region (%d launches); the kernel runs alone there' % roof['launches']
        else:
            rf['measured'] = ('HIP events on the launch stream in %d single-stream steps after the timed region (%d launches): in the '
                              'real step this kernel overlaps the kernels of the other backward stream (data-gradients on the main stream, weight gradients on the second), where a launch took '
                              '%.1f us on average (overlapped, not a per-kernel figure)'
                              % (roof_steps, roof['launches'], timed[dom]['avg_us']))
        # the committed PMC pass was taken on the default configuration only
        tr, src = pmc_traffic(args.workload, dom) if (args.tpad == 1600 and args.batch == 32) else (None, None)
        rf['traffic'] = tr
        if src:
            rf['traffic_unit'] = 'bytes/launch (PMC pass: %s)' % src
        if args.kernel_table:
            for key, r in sorted(table.items(), key=lambda kv: -kv[1]['total_ms']):
                pk, ex, _ = kernel_peak(key)
                print('%-56s launches %3d  total %8.3f ms  avg %9.1f us  %7.2f TFLOP/s algorithmic  %.3f of the fp32 pipe (executed flops)' %
                      (key, r['launches'], r['total_ms'], r['avg_us'], r['tflops'], r['tflops'] * ex / pk), file=sys.stderr)
        if not args.no_cpu_baseline and world == 1:
            out['cpu_baseline'] = cpu_baseline(variant, T, V, batch=B)
        print(json.dumps(out), flush=True)
    barrier()
    if dist.is_initialized():
        shutdown_process_group()


if __name__ == '__main__':
    sys.exit(main() or 0)
