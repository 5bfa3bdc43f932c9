#!/usr/bin/env python3
"""Reference-shaped training / evaluation driver on synthetic videos.

Follows the iteration protocol of the reference's train.py (:253-331) with the same module calls:
  tap_feats, pred_proposals = tap_model(c3d_feats)                                   (:285)
  pred = cg_model(tap_feats, c3d_feats, lda_feats, cg_labels, ind, soi, mode='train') (:298)
  cg_loss = LanguageModelCriterion()(pred, labels[:, 1:], masks[:, 1:])               (:300)
  total = lambda1 * tap_loss + lambda2 * cg_loss  ('tap_cg' joint mode, :322-329), backward,
  clip_gradient + optimizer.step every m_batch videos (:281-283,313-317), step LR decay (:232-240),
and saves checkpoints in the reference's dict layout (:456-461) so that either code base can resume the other's run.
Both models run natively (echr_amd's SST: echr_sst_fwd/bwd; the caption path: echr_tsrm_* / echr_decoder_*), both optimisers are
the fused ClampAdam, and `--resume` restores models AND optimiser state (train.py:214-216).

`--pre_tap` is stage 1 of the reference's recipe (experiments/train_SST.sh, training_mode 'pre_tap'): the proposal encoder alone, the
gradients of m_batch videos summed before one clamp + step.  Here the m_batch videos are ONE call: tap_model.forward_batch over the
concatenated features, utils.tap_criterion_batch (every video its own mean), one backward, one fused step.

`--joint --m_batch V` (V > 1) is stage 3 (finetune.sh, training_mode 'tap_cg') with the V videos of one accumulation as ONE batch:
fused.JointBatchStep -- the proposal encoder, both criteria, the caption side with d loss / d tap_feats, both backward passes and one clamp +
Adam per model, without an autograd graph (`--no-fused` keeps the V sequential autograd iterations with accumulation).  In this mode, as
with `--pre_tap`, ONE iteration of `--iters` is one batch of V videos with an update, and the `iteration` that `--save` writes counts such
batches; the autograd modes count single-video iterations (an update every m_batch of them), so a checkpoint resumed under the other mode
continues at a different video and epoch.

`--self_critical` is the stage past `--self_critical_after` (train.py:241-245, 303-308): a sampled and a greedy caption per event, the
reward-weighted step on the sample.  m_batch = 1 runs fused.SelfCriticalStep per video, m_batch = V > 1 runs fused.SelfCriticalBatchStep on
the V videos of one accumulation as ONE batch (one iteration of `--iters` is then one batch with an update).  The reward is synthetic:
the token overlap of the sampled caption with the video's ground-truth caption minus the same for the greedy caption.

Under `torchrun --nproc_per_node R` (RANK / WORLD_SIZE in the environment) with `--m_batch V` (V > 1) the V videos of an update are sharded
over the R ranks (parallel.shard_batch) and every rank runs fused.DataParallelBatchStep around the stage's batch step -- FusedTrainStep's
batch form, JointBatchStep with `--joint`, SelfCriticalBatchStep with `--self_critical`: gradients and loss are the sum over all videos of all
ranks, one clamp + Adam per model, identical on every rank.  `--dist_backend gloo` with fewer devices than ranks is the one-GPU rehearsal:
every rank on cuda:0, launch-per-phase recurrences.  Without a process group nothing changes.

`--caption_model show_attend_tell --CG_input_feats_type VEC` trains the reference's default one-stream decoder (one LSTM layer, echr_amd.sat)
on the plain autograd path -- forward, criterion, backward, clip_gradient, ClampAdam.step over the flat arena -- and decodes greedily.
With `--m_batch V` (V > 1, without --joint) the V videos of an update are ONE VideoBatch built for that decoder: forward_batch,
batch.criterion, backward, clip_gradient, ClampAdam.step -- the launch chain of the decoder once per update instead of once per video.

`--gt_targets` (with `--joint --m_batch V` or `--pre_tap`) trains from ground-truth SEGMENTS instead of ready-made supervision: the loader's
videos carry featstamps and one caption per segment (synth.make_gt_video), and every batch's proposal labels, masks and caption events are
built on the device by echr_amd.targets.build (dataloader.get_vid_data / get_shuffle_list: IoU of every anchor against every segment, the
thresholded maps, a sample of `--events` good proposals per video, a new draw every iteration).  Videos without a good proposal are skipped
as train.py:261 does.

`--ext_proposals P` makes the evaluation leg caption P synthetic external proposals of video 0 -- (start s, end s) segments with a score each,
as a temporal-event-proposal file gives them -- through eval_utils.caption_video(flag_eval_what='SOTA_TEP', ext_proposals=...): greedy cluster
NMS over the timestamps, topN, featstamps and the crop of over-long proposals on the device (echr_amd.extprops).

usage: python examples/train_synthetic.py [--iters 20] [--m_batch 2] [--joint] [--pre_tap] [--self_critical [--reward ciderd]] [--save /tmp/echr_ckpt.pth]
                                          [--resume /tmp/echr_ckpt.pth]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import echr_amd
from echr_amd import models, synth
from echr_amd.misc import utils
from echr_amd.optim import ClampAdam


def make_loader(opt, n_videos, N, A, L, seed=0):
    V1 = opt.CG_vocab_size + 1
    vids = [synth.make_video(N, A, L, V1, seed=seed + i, video_dim=opt.video_dim, hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim)
            for i in range(n_videos)]
    rs = np.random.RandomState(seed)
    for v in vids:       # proposal labels / masks / class weights of the SST head (shapes as dataloader.py:320-365 produces them)
        T = v['T_v']
        v['tap_labels'] = (rs.uniform(size=(T, opt.K)) > 0.9).astype(np.float32)
        v['tap_masks'] = (np.arange(T)[:, None] >= np.arange(opt.K)[None, :]).astype(np.float32)
        v['w1'] = rs.uniform(0.05, 0.3, size=(opt.K,)).astype(np.float32)
    return vids


def make_gt_loader(opt, n_videos, G, A, L, seed=0):
    """--gt_targets: annotated videos as a dataset gives them -- G ground-truth segments of up to min(A, K) - 2 rows with one caption each
    on a video of A + max(8, A // 4) rows (make_video's default length), and the class weights of the SST head."""
    V1 = opt.CG_vocab_size + 1
    vids = [synth.make_gt_video(A + max(8, A // 4), G, L, V1, seed=seed + i, max_len=max(2, min(A, opt.K) - 2), video_dim=opt.video_dim,
                                hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim) for i in range(n_videos)]
    rs = np.random.RandomState(seed)
    for v in vids:
        v['w1'] = rs.uniform(0.05, 0.3, size=(opt.K,)).astype(np.float32)
    return vids


def build_targets(a, opt, dev, vids, it):
    """The batch's supervision from its segments (echr_amd.targets.build): a new sample per iteration through the draw ids."""
    from echr_amd import targets
    return targets.build(vids, opt.K, prop_sample_num=a.events, seed=a.target_seed, device=dev,
                         draw=[(it * a.m_batch + j) % (1 << 31) for j in range(len(vids))])


def set_lr_for_epoch(optimizer, base_lr, epoch, start=8, every=3, rate=0.5):
    """Step decay as train.py:232-240."""
    lr = base_lr if epoch <= start or start < 0 else base_lr * rate ** ((epoch - start) // every)
    utils.set_lr(optimizer, lr)
    return lr


def save_checkpoint(path, iteration, cg_model, tap_model, cg_opt, tap_opt):
    torch.save({'iteration': iteration, 'cg_model': cg_model.state_dict(), 'tap_model': tap_model.state_dict(),
                'cg_optimizer': cg_opt.state_dict(), 'tap_optimizer': tap_opt.state_dict()}, path)


def pre_tap(a, opt, dev, loader, tap_model, cg_model, cg_opt, tap_opt, tap_crit, start):
    """Stage 1: the SST alone over m_batch videos per call (train.py:281-283,313-317 with the videos of one accumulation as one batch)."""
    as_dev = lambda vids, k: torch.from_numpy(np.concatenate([v[k] for v in vids], 0)).to(dev)
    history = []
    for it in range(start, start + a.iters):
        vids = [loader[(it * a.m_batch + j) % len(loader)] for j in range(a.m_batch)]
        set_lr_for_epoch(tap_opt, opt.lr, it * a.m_batch // len(loader))
        row_offset = np.concatenate([[0], np.cumsum([len(v['c3d']) for v in vids])])
        tap_opt.zero_grad()
        _, pred_proposals = tap_model.forward_batch(as_dev(vids, 'c3d'), row_offset)
        if a.gt_targets:          # labels and masks built on the device from the videos' segments
            t = build_targets(a, opt, dev, vids, it)
            masks, labels = t.tap_masks, t.tap_labels
        else:
            masks, labels = as_dev(vids, 'tap_masks'), as_dev(vids, 'tap_labels')
        tap_loss, per_video = utils.tap_criterion_batch(tap_crit, pred_proposals, masks, labels,
                                                        [torch.from_numpy(v['w1']).to(dev) for v in vids], row_offset)
        tap_loss.backward()
        utils.clip_gradient(tap_opt, opt.grad_clip)
        tap_opt.step()
        history.append(float(tap_loss.detach()) / a.m_batch)
        if not a.quiet and (it % 5 == 0 or it == start + a.iters - 1):
            print('iter %3d  tap_loss %.4f  (mean of %d videos)' % (it, history[-1], a.m_batch), flush=True)
    if a.save:
        save_checkpoint(a.save, start + a.iters, cg_model, tap_model, cg_opt, tap_opt)
    return history, cg_model, tap_model


def init_distributed(a):
    """torchrun's process group (None without RANK / WORLD_SIZE): RCCL with one device per rank, or the gloo rehearsal on a shared device."""
    if 'RANK' not in os.environ or 'WORLD_SIZE' not in os.environ:
        return None
    import torch.distributed as dist
    from echr_amd import _lib
    rank, world, local = int(os.environ['RANK']), int(os.environ['WORLD_SIZE']), int(os.environ.get('LOCAL_RANK', '0'))
    shared = torch.cuda.device_count() < world
    if shared and a.dist_backend != 'gloo':
        raise SystemExit('%d ranks on %d device(s): RCCL wants one device per rank (--dist_backend gloo rehearses on a shared one)'
                         % (world, torch.cuda.device_count()))
    torch.cuda.set_device(0 if shared else local)
    _lib.check(_lib.load().echr_streams_init(), 'streams_init')          # (the library's helper streams ahead of the communicator: INTEGRATION.md)
    if a.dist_backend == 'nccl':
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', local))
    else:
        dist.init_process_group(a.dist_backend, rank=rank, world_size=world)
    if shared:          # two ranks' persistent grids must never share a device: launch-per-phase recurrences and proposal encoder
        for key in (b'persist', b'persist_bwd', b'sst_persist'):
            _lib.check(_lib.load().echr_config_set(key, 0), 'config_set')
    return rank, world


def data_parallel_batch(a, opt, dev, loader, tap_model, cg_model, cg_opt, tap_opt, start, rank, world):
    """`--m_batch V` under a process group: the V videos of an update sharded over the ranks, fused.DataParallelBatchStep around the stage's
    batch step (train.py:281-283,313-317 with the m_batch videos on R ranks).  Every rank prints the same, reduced loss."""
    from echr_amd import parallel
    from echr_amd.batch import VideoBatch
    from echr_amd.fused import DataParallelBatchStep, FusedTrainStep, JointBatchStep, SelfCriticalBatchStep
    fused = FusedTrainStep(cg_model, cg_opt, grad_clip=opt.grad_clip)
    keys = ('c3d', 'lda', 'ind', 'soi', 'labels', 'masks')
    rewards = []
    if a.joint:
        inner, stage = JointBatchStep(fused, tap_model, tap_opt, lambda1=0.01, lambda2=1.0, tap_grad_clip=opt.grad_clip), 'JointBatchStep'
    elif a.self_critical:
        inner, stage = SelfCriticalBatchStep(fused, lambda gen, greedy: rewards[inner.current_video](gen, greedy)), 'SelfCriticalBatchStep'
    else:
        inner, stage = fused, 'FusedTrainStep.batch'
    dp = DataParallelBatchStep(inner, reduce_loss=True)
    history = []
    for it in range(start, start + a.iters):
        vids = parallel.shard_batch([loader[(it * a.m_batch + j) % len(loader)] for j in range(a.m_batch)], rank, world)
        epoch = it * a.m_batch // len(loader)
        set_lr_for_epoch(cg_opt, opt.lr, epoch)
        if a.joint:
            set_lr_for_epoch(tap_opt, opt.lr, epoch)
        if not vids:          # fewer videos than ranks: this rank adds zeros and takes part in every collective and in the update
            loss = dp(None)
        elif a.joint:
            loss = dp([{k: v[k] for k in keys} for v in vids], [torch.from_numpy(v['tap_masks']) for v in vids],
                      [torch.from_numpy(v['tap_labels']) for v in vids], [torch.from_numpy(v['w1']) for v in vids])
        else:
            with torch.no_grad():          # the proposal encoder is idle in these stages: its states carry no graph
                batch = VideoBatch.from_videos([{k: v[k] for k in (keys[:4] if a.self_critical else keys)} for v in vids], device=dev,
                                               tap_model=tap_model, clip_context_type=opt.clip_context_type,
                                               CG_init_feats_type=opt.CG_init_feats_type)
            rewards[:] = [overlap_reward(v['labels']) for v in vids]
            loss = dp(batch)
        history.append(float(loss) / a.m_batch)
        if not a.quiet and rank == 0 and (it % 5 == 0 or it == start + a.iters - 1):
            print('iter %3d  DataParallelBatchStep(%s) over %d videos on %d ranks: loss %.4f  (mean over the videos; %d collectives, %d early)'
                  % (it, stage, a.m_batch, world, history[-1], dp.n_collectives, dp.n_early), flush=True)
    return history


def joint_batch(a, opt, dev, loader, tap_model, cg_model, cg_opt, tap_opt, start):
    """Stage 3 ('tap_cg') over m_batch videos per call: one fused.JointBatchStep call per accumulation (train.py:281-329 with the videos of one
    accumulation as one batch; lambda1 = 0.01, lambda2 = 1 as opts.py:194-196)."""
    from echr_amd.fused import FusedTrainStep, JointBatchStep
    step = JointBatchStep(FusedTrainStep(cg_model, cg_opt, grad_clip=opt.grad_clip), tap_model, tap_opt, lambda1=0.01, lambda2=1.0,
                          tap_grad_clip=opt.grad_clip)
    keys = ('c3d', 'lda', 'ind', 'soi', 'labels', 'masks')
    history = []
    for it in range(start, start + a.iters):
        vids = [loader[(it * a.m_batch + j) % len(loader)] for j in range(a.m_batch)]
        epoch = it * a.m_batch // len(loader)
        set_lr_for_epoch(cg_opt, opt.lr, epoch)
        set_lr_for_epoch(tap_opt, opt.lr, epoch)
        if a.gt_targets:          # proposal labels, masks and the sampled caption events built on the device from the videos' segments
            t = build_targets(a, opt, dev, vids, it)
            videos = t.videos([{k: v[k] for k in keys[:2]} for v in vids], [v['gt_labels'] for v in vids], [v['gt_masks'] for v in vids])
            if not videos:          # no video of the batch has a good proposal (train.py:261)
                continue
            loss = step(videos, t.kept(t.tap_masks), t.kept(t.tap_labels), [torch.from_numpy(vids[v]['w1']) for v in t.keep])
        else:
            loss = step([{k: v[k] for k in keys} for v in vids], [torch.from_numpy(v['tap_masks']) for v in vids],
                        [torch.from_numpy(v['tap_labels']) for v in vids], [torch.from_numpy(v['w1']) for v in vids])
        history.append(float(step.cg_loss) / a.m_batch)
        if not a.quiet and (it % 5 == 0 or it == start + a.iters - 1):
            print('iter %3d  JointBatchStep over %d videos: joint_loss %.4f  cg_loss %.4f  tap_loss %.4f  (means over the videos)'
                  % (it, a.m_batch, float(loss) / a.m_batch, history[-1], float(step.tap_loss) / a.m_batch), flush=True)
    return history


def overlap_reward(labels):
    """reward_fn of the self-critical steps for events with the ground-truth `labels` [N, L] (host, <bos> in column 0): per caption, the
    fraction of its tokens that occur in the event's ground-truth caption, sampled minus greedy (a stand-in for CIDEr differences)."""
    truth = [set(int(t) for t in row[1:] if t > 0) for row in np.asarray(labels)]

    def score(seq):
        out = np.zeros(len(truth), np.float32)
        for n, row in enumerate(np.asarray(seq)):
            toks = [int(t) for t in row if t > 0]
            out[n] = sum(t in truth[n] for t in toks) / max(len(toks), 1)
        return out
    return lambda gen, greedy: score(gen) - score(greedy)


def self_critical(a, opt, dev, loader, tap_model, cg_model, cg_opt, start):
    """Self-critical training of the captioner (the proposal encoder idle, its states without a graph): SelfCriticalStep per video, or
    SelfCriticalBatchStep over the m_batch videos of one accumulation as one batch."""
    from echr_amd.batch import VideoBatch
    from echr_amd.fused import FusedTrainStep, SelfCriticalBatchStep, SelfCriticalStep
    fused = FusedTrainStep(cg_model, cg_opt, grad_clip=opt.grad_clip)
    ciderd = None
    if a.reward == 'ciderd':
        # CIDEr-D on the device: the corpus is every synthetic video's labels (one document per event), an event's reference its own label;
        # the references are packed and uploaded once per video, outside the iterations
        from echr_amd.reward import CiderD, CiderDReward
        scorer = CiderD.from_corpus([[lab] for v in loader for lab in np.asarray(v['labels'])], opt.CG_seq_length, opt.CG_vocab_size).to(dev)
        ciderd = CiderDReward(scorer)
        packed = {id(v): scorer.pack_refs([[lab] for lab in np.asarray(v['labels'])]).to(dev) for v in loader}
        one, many = SelfCriticalStep(fused, ciderd), SelfCriticalBatchStep(fused, ciderd)
    history = []
    for it in range(start, start + a.iters):
        vids = [loader[(it * a.m_batch + j) % len(loader)] for j in range(a.m_batch)]
        set_lr_for_epoch(cg_opt, opt.lr, it * a.m_batch // len(loader))
        if a.m_batch == 1:
            v = vids[0]
            c3d, lda = torch.from_numpy(v['c3d']).to(dev), torch.from_numpy(v['lda']).to(dev)
            with torch.no_grad():
                tap_feats, _ = tap_model(c3d)
            if ciderd is not None:
                loss = one(tap_feats, c3d, lda, v['ind'], v['soi'], refs=packed[id(v)])[0]
            else:
                loss = SelfCriticalStep(fused, overlap_reward(v['labels']))(tap_feats, c3d, lda, v['ind'], v['soi'])[0]
        else:
            rewards = [overlap_reward(v['labels']) for v in vids]          # reward_fn is called once per video (step.current_video)
            with torch.no_grad():
                batch = VideoBatch.from_videos([{k: v[k] for k in ('c3d', 'lda', 'ind', 'soi')} for v in vids], device=dev, tap_model=tap_model,
                                                 clip_context_type=opt.clip_context_type, CG_init_feats_type=opt.CG_init_feats_type)
            if ciderd is not None:          # the batch's references: its videos' packed rows in batch order
                from echr_amd.reward import PackedRefs
                parts = [packed[id(v)] for v in vids]
                base = np.cumsum([0] + [int(p.refs.shape[0]) for p in parts])
                refs = PackedRefs(torch.cat([p.refs for p in parts]), torch.cat([p.ref_len for p in parts]),
                                  torch.cat([parts[0].ref_offset[:1]] + [p.ref_offset[1:] + int(o) for p, o in zip(parts, base)]))
                batch.refs = refs
                loss = many(batch)[0]
            else:
                step = SelfCriticalBatchStep(fused, lambda gen, greedy: rewards[step.current_video](gen, greedy))
                loss = step(batch)[0]
        history.append(float(loss) / a.m_batch)
        if not a.quiet and (it % 5 == 0 or it == start + a.iters - 1):
            print('iter %3d  self-critical loss %.4f  (mean of %d videos)' % (it, history[-1], a.m_batch), flush=True)
    return history


def one_stream_batch(a, opt, dev, loader, tap_model, cg_model, cg_opt, cg_crit, start):
    """--caption_model show_attend_tell --m_batch V ('pre_cg' mode: the proposal encoder idle, its states without a graph): the V videos of an
    update as one VideoBatch through forward_batch + batch.criterion + backward + clip_gradient + ClampAdam.step."""
    from echr_amd.batch import VideoBatch
    history = []
    for it in range(start, start + a.iters):
        vids = [loader[(it * a.m_batch + j) % len(loader)] for j in range(a.m_batch)]
        set_lr_for_epoch(cg_opt, opt.lr, it * a.m_batch // len(loader))
        cg_opt.zero_grad()
        with torch.no_grad():
            batch = VideoBatch.from_videos([{k: v[k] for k in ('c3d', 'lda', 'ind', 'soi', 'labels', 'masks')} for v in vids], device=dev,
                                             tap_model=tap_model, clip_context_type=opt.clip_context_type,
                                             CG_init_feats_type=opt.CG_init_feats_type, caption_model=opt.caption_model)
        pred = cg_model.forward_batch(batch, mode='train')
        loss, _ = batch.criterion(cg_crit, pred)
        loss.backward()
        utils.clip_gradient(cg_opt, opt.grad_clip)
        cg_opt.step()
        history.append(float(loss.detach()) / a.m_batch)
        if not a.quiet and (it % 5 == 0 or it == start + a.iters - 1):
            print('iter %3d  cg_loss %.4f  (mean of %d videos, one forward_batch call)' % (it, history[-1], a.m_batch), flush=True)
    return history


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--m_batch', type=int, default=1)
    ap.add_argument('--joint', action='store_true', help="'tap_cg' mode: gradients flow through tap_feats into the SST")
    ap.add_argument('--pre_tap', action='store_true', help="'pre_tap' mode: train the proposal encoder alone, m_batch videos per forward_batch call")
    ap.add_argument('--self_critical', action='store_true', help='self-critical training of the captioner: SelfCriticalStep (m_batch = 1) or '
                                                                 'SelfCriticalBatchStep over the m_batch videos as one batch')
    ap.add_argument('--reward', choices=('overlap', 'ciderd'), default='overlap', help="--self_critical: the host stand-in overlap_reward, or "
                                                                                       "CIDEr-D scored on the device (echr_amd.reward) against "
                                                                                       "each event's own label")
    ap.add_argument('--events', type=int, default=16)
    ap.add_argument('--gt_targets', action='store_true', help='with --joint --m_batch V or --pre_tap: the loader gives ground-truth segments '
                                                              'with one caption each, and every batch\'s proposal labels, masks and '
                                                              '--events sampled caption events are built on the device (echr_amd.targets)')
    ap.add_argument('--gt_segments', type=int, default=4, help='--gt_targets: ground-truth segments per synthetic video')
    ap.add_argument('--target_seed', type=int, default=0, help='--gt_targets: the key of the proposal sampling')
    ap.add_argument('--ext_proposals', type=int, default=0, metavar='P', help="the evaluation leg captions P synthetic EXTERNAL proposals of "
                                                                              "video 0 (seconds + scores; flag_eval_what='SOTA_TEP') instead of its ready-made events")
    ap.add_argument('--segments', type=int, default=32)
    ap.add_argument('--vocab', type=int, default=500)
    ap.add_argument('--lr', type=float, default=5e-4)
    ap.add_argument('--clip_context_type', type=str, default='CC', help="frame-level context: 'CC', 'CH' or 'CC+CH' (opts.py:130); the batches of "
                                                                        "--m_batch V are built for it")
    ap.add_argument('--CG_init_feats_type', type=str, default='', help="non-zero initial decoder state from 'V', 'E', 'C' (opts.py); the batches "
                                                                       "of --m_batch V are built for it")
    ap.add_argument('--caption_model', type=str, default='three_stream', help="'three_stream' (the ECHR recipe) or 'show_attend_tell' (the "
                                                                                "reference's default one-stream decoder, one LSTM layer: trains "
                                                                                "on the plain autograd path, one video per call)")
    ap.add_argument('--CG_input_feats_type', type=str, default='', help="show_attend_tell: the contexts its LSTM reads beside the token, from "
                                                                        "'V', 'E', 'C' (e.g. VEC)")
    ap.add_argument('--dist_backend', type=str, default='nccl', help="under torchrun: 'nccl' (RCCL, one device per rank) or 'gloo' (also the "
                                                                     "rehearsal with every rank on one device)")
    ap.add_argument('--save', type=str, default='')
    ap.add_argument('--resume', type=str, default='', help='checkpoint written by --save (or by the reference): models + optimiser state')
    ap.add_argument('--quiet', action='store_true')
    ap.add_argument('--no-fused', action='store_true', help="keep the autograd path also where one echr_train_step call per iteration applies "
                                                             "('pre_cg' mode with m_batch = 1)")
    a = ap.parse_args(argv)
    if 'RANK' in os.environ and 'WORLD_SIZE' in os.environ and (a.m_batch < 2 or a.no_fused or a.pre_tap):
        # every rank would train its own replica on the single-process path, without any exchange
        raise SystemExit('under torchrun this driver runs fused.DataParallelBatchStep: it needs --m_batch V with V > 1 and takes neither '
                         '--no-fused nor --pre_tap')
    ranks = init_distributed(a)
    dev = torch.device('cuda')
    opt = synth.default_opt(vocab_size=a.vocab, seq_length=10, K=32, lr=a.lr)
    opt.clip_context_type = a.clip_context_type
    opt.CG_init_feats_type = a.CG_init_feats_type
    if a.caption_model == 'show_attend_tell':
        # the one-stream decoder has no one-call step or self-critical entry yet: forward / forward_batch, criterion, backward, clip, ClampAdam.step
        if a.self_critical or 'RANK' in os.environ or (a.joint and a.m_batch > 1 and not a.no_fused):
            raise SystemExit('--caption_model show_attend_tell trains on the autograd path: not with --self_critical, torchrun or the batched --joint')
        opt.caption_model, opt.CG_num_layers, opt.CG_input_feats_type = 'show_attend_tell', 1, a.CG_input_feats_type
        a.no_fused = True
    elif a.caption_model != 'three_stream':
        raise SystemExit("--caption_model is 'three_stream' or 'show_attend_tell'")
    torch.manual_seed(0)
    tap_model = models.setup_tap(opt).to(dev)
    cg_model = echr_amd.CaptionGenerator(opt).to(dev)
    tap_model.train()
    cg_model.train()
    batch_joint = a.joint and a.m_batch > 1 and not a.no_fused and not a.pre_tap          # stage 3 over a batch: fused.JointBatchStep
    dp_batch = ranks is not None and a.m_batch > 1 and not a.no_fused and not a.pre_tap          # ... and any stage's batch step over the ranks
    tap_opt = ClampAdam(tap_model.parameters(), lr=opt.lr, betas=(opt.optim_alpha, opt.optim_beta), eps=opt.optim_epsilon,
                        arena=tap_model.build_arena() if batch_joint else None)
    cg_opt = ClampAdam(cg_model.parameters(), lr=opt.lr, betas=(opt.optim_alpha, opt.optim_beta), eps=opt.optim_epsilon,
                       arena=cg_model.build_arena())
    # the reference clamps the running gradient after EVERY backward (train.py:315-317); ClampAdam keeps that trajectory for any m_batch
    # (the clamp deferred to the fused step kernel is applied first whenever another backward accumulates)
    start = 0
    if a.resume:
        ck = torch.load(a.resume, map_location=dev)
        cg_model.load_state_dict(ck['cg_model'])
        tap_model.load_state_dict(ck['tap_model'])
        cg_opt.load_state_dict(ck['cg_optimizer'])
        tap_opt.load_state_dict(ck['tap_optimizer'])
        start = int(ck['iteration'])
    cg_crit, tap_crit = utils.LanguageModelCriterion(), utils.TAPModelCriterion()
    # 'pre_cg' mode (train_ECHR.sh) with m_batch = 1: the whole iteration around the caption model -- zero_grad, forward, criterion,
    # backward, clip_gradient, step (train.py:281-317) -- is ONE library call
    # 'tap_cg' mode with m_batch = 1: the caption side is the same call; d loss / d tap_feats comes back in tap_grad and goes into the proposal
    # encoder together with its own loss, cg_model's parameter gradients + Adam finish on the library's helper streams meanwhile
    fused = None
    if a.m_batch == 1 and not a.no_fused:
        from echr_amd.fused import FusedTrainStep
        fused = FusedTrainStep(cg_model, cg_opt, grad_clip=opt.grad_clip)
    if a.gt_targets and not (a.pre_tap or (batch_joint and not dp_batch)):
        raise SystemExit('--gt_targets builds the targets of a batch: it goes with --joint --m_batch V (V > 1) or --pre_tap in one process')
    if a.gt_targets:
        loader = make_gt_loader(opt, 8, a.gt_segments, a.segments, opt.CG_seq_length + 2)
    else:
        loader = make_loader(opt, 8, a.events, a.segments, opt.CG_seq_length + 2)
    history = []
    if a.pre_tap:
        return pre_tap(a, opt, dev, loader, tap_model, cg_model, cg_opt, tap_opt, tap_crit, start)
    iters = range(start, start + a.iters)
    if a.self_critical and (a.joint or a.no_fused):
        raise SystemExit('--self_critical trains the captioner on the one-call path: not with --joint / --no-fused')
    if a.reward == 'ciderd' and (not a.self_critical or dp_batch):
        raise SystemExit('--reward ciderd goes with --self_critical in one process (the data-parallel driver keeps overlap_reward)')
    if a.self_critical and not dp_batch:
        history, iters = self_critical(a, opt, dev, loader, tap_model, cg_model, cg_opt, start), ()
    if dp_batch:
        history, iters = data_parallel_batch(a, opt, dev, loader, tap_model, cg_model, cg_opt, tap_opt, start, *ranks), ()
    elif batch_joint:
        history, iters = joint_batch(a, opt, dev, loader, tap_model, cg_model, cg_opt, tap_opt, start), ()
    elif a.caption_model == 'show_attend_tell' and a.m_batch > 1 and not a.joint:
        history, iters = one_stream_batch(a, opt, dev, loader, tap_model, cg_model, cg_opt, cg_crit, start), ()
    for it in iters:
        v = loader[it % len(loader)]
        set_lr_for_epoch(cg_opt, opt.lr, it // len(loader))
        c3d, lda = torch.from_numpy(v['c3d']).to(dev), torch.from_numpy(v['lda']).to(dev)
        if fused is not None and a.joint:
            tap_opt.zero_grad()
            tap_feats, pred_proposals = tap_model(c3d)
            tap_loss = 0.01 * tap_crit(pred_proposals, torch.from_numpy(v['tap_masks']).to(dev), torch.from_numpy(v['tap_labels']).to(dev),
                                       torch.from_numpy(v['w1']).to(dev))                       # lambda1 (opts.py:194-196); lambda2 = 1
            g_tap = torch.zeros_like(tap_feats)
            cg_loss = fused(tap_feats.detach(), c3d, lda, v['labels'], v['ind'], v['soi'], torch.from_numpy(v['labels'])[:, 1:],
                            torch.from_numpy(v['masks'])[:, 1:], tap_grad=g_tap, defer_update=True)
            torch.autograd.backward([tap_loss, tap_feats], [None, g_tap])
            utils.clip_gradient(tap_opt, opt.grad_clip)
            tap_opt.step()
            history.append(float(cg_loss))
            if not a.quiet and (it % 5 == 0 or it == start + a.iters - 1):
                print('iter %3d  cg_loss %.4f' % (it, history[-1]), flush=True)
            continue
        if fused is not None:
            with torch.no_grad():
                tap_feats, _ = tap_model(c3d)
            cg_loss = fused(tap_feats, c3d, lda, v['labels'], v['ind'], v['soi'], torch.from_numpy(v['labels'])[:, 1:], torch.from_numpy(v['masks'])[:, 1:])
            history.append(float(cg_loss))
            if not a.quiet and (it % 5 == 0 or it == start + a.iters - 1):
                print('iter %3d  cg_loss %.4f' % (it, history[-1]), flush=True)
            continue
        if it % a.m_batch == 0:
            cg_opt.zero_grad()
            tap_opt.zero_grad()
        tap_feats, pred_proposals = tap_model(c3d)
        if not a.joint:
            tap_feats = tap_feats.detach()                                       # 'pre_cg' mode: the proposal net is idle
        pred = cg_model(tap_feats, c3d, lda, v['labels'], v['ind'], v['soi'], mode='train')
        cg_loss = cg_crit(pred, torch.from_numpy(v['labels'])[:, 1:].to(dev), torch.from_numpy(v['masks'])[:, 1:].to(dev))
        loss = cg_loss
        if a.joint:
            tap_loss = tap_crit(pred_proposals, torch.from_numpy(v['tap_masks']).to(dev), torch.from_numpy(v['tap_labels']).to(dev),
                                torch.from_numpy(v['w1']).to(dev))
            loss = 0.01 * tap_loss + 1.0 * cg_loss                                # lambda1, lambda2 defaults (opts.py:194-196)
        loss.backward()
        utils.clip_gradient(cg_opt, opt.grad_clip)                                # after every backward, as train.py:315,325-326
        if a.joint:
            utils.clip_gradient(tap_opt, opt.grad_clip)
        if (it + 1) % a.m_batch == 0:
            cg_opt.step()
            if a.joint:
                tap_opt.step()
        history.append(float(cg_loss.detach()))
        if not a.quiet and (it % 5 == 0 or it == start + a.iters - 1):
            print('iter %3d  cg_loss %.4f' % (it, history[-1]), flush=True)
    if fused is not None:
        fused.join()                                                              # a deferred update of the last iteration
    cg_model.eval()
    with torch.no_grad():
        v = loader[0]
        c3d, lda = torch.from_numpy(v['c3d']).to(dev), torch.from_numpy(v['lda']).to(dev)
        tap_model.eval()
        tap_feats, _ = tap_model(c3d)
        if a.gt_targets:          # caption the ground-truth events (the reference's gts_*_select_list)
            from echr_amd import targets
            v = dict(v, **targets.gt_events(v['featstamps']))
        if a.ext_proposals:          # somebody else's proposals: NMS over the timestamps, score threshold, topN, featstamps, crop (extprops.select)
            from echr_amd import eval_utils
            rs = np.random.RandomState(a.target_seed)
            start_s = rs.uniform(0.0, 50.0, size=a.ext_proposals)
            stamps = np.stack([start_s, start_s + rs.uniform(1.0, 30.0, size=a.ext_proposals)], 1)
            info, extras = eval_utils.caption_video(tap_model, cg_model, c3d, lda, 60.0, None, flag_eval_what='SOTA_TEP', topN=8, nms_threshold=0.7,
                                                    ext_proposals=(stamps, rs.permutation(a.ext_proposals) / float(a.ext_proposals)),
                                                    ext_seed=a.target_seed)
            seq = extras['seq'] if extras['seq'] is not None else []
            if not a.quiet:
                print('external proposals: %d of %d selected, rows' % (len(extras['soi_select_list']), a.ext_proposals), extras['soi_select_list'][:3])
                print('captioned (seconds, score):', [(r['timestamp'], round(r['proposal_score'], 3)) for r in info[:3]])
        else:
            seq, logp = cg_model(tap_feats, c3d, lda, [], v['ind'], v['soi'], mode='eval')
    if not a.quiet:
        print('greedy captions (token ids) of video 0:', seq[:3].tolist() if len(seq) else seq)
    if a.save and (ranks is None or ranks[0] == 0):
        save_checkpoint(a.save, start + a.iters, cg_model, tap_model, cg_opt, tap_opt)
    if ranks is not None:
        import torch.distributed as dist
        dist.destroy_process_group()
    return history, cg_model, tap_model


if __name__ == '__main__':
    main()
