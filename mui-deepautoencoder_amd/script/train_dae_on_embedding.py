#!/usr/bin/env python3
"""Train the embedding denoising autoencoder on MI355X.

Same command line, config schema, data split, log lines and outputs as the reference's
script/train_dae_on_embedding.py (--embedding_path --output_path --config [--debug --rank
--nb_missing]); the inner loop (reference :194-223 and :241-261) is one fused HIP step per
minibatch over the HBM-resident dataset (codae.train.HipEmbeddingTrainer) instead of
DataLoader + per-sample mask loop + autograd + per-step host copies.

Checkpoints: `HIP: CHECKPOINT: {EVERY: 1, KEEP: 2, DIR: <the run's output directory>}` writes checkpoint_epoch<k>.npz after every
EVERY-th epoch's validation sweep and keeps the newest KEEP; --resume PATH continues such a file's run at its next epoch, bit for bit
the run that was never interrupted (codae.train.HipEmbeddingTrainer.save / load).

Outfit codes: `HIP: CODES: {SAVE: true, LAYER: null, NEIGHBOURS: 0, DISTINCT: true}` writes codes.npz - every dataset row's latent
vector and, with NEIGHBOURS k > 0, its k nearest other rows in code space - into the run's output directory after the last epoch
(codae.train.HipEmbeddingTrainer.code_index, codae.tool.OutfitCodes).

Code clusters: `HIP: CODE_CLUSTERS: {K: 64, ITERS: 25, SEED: 0, LAYER: null}` clusters those codes by spherical k-means on the device
and writes clusters.npz - centroids, every row's cluster and score, counts, objective, changed - beside it (codae.tool.CodeClusters).

Extra flags: --precision {bf16,f32} (default: HIP.PRECISION of the config, else bf16; widths the
bf16 tiles cannot take fall back to the exact-fp32 kernels), --epochs N (override MODEL.EPOCH).
Multi-GPU: launch with `python -m torch.distributed.run --nproc-per-node N`; each rank takes
1/N of every minibatch and gradients are all-reduced over RCCL.
"""
import argparse
import logging
import math
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from codae.hostcpu import cap_thread_env                                   # noqa: E402
cap_thread_env()        # BLAS / OpenMP pools no wider than the container's CPU quota, before numpy and torch create them

import numpy as np                                                       # noqa: E402
import torch
import yaml


from codae.hip import HipError                                            # noqa: E402
from codae.model.schedule import linear_stack                             # noqa: E402
from codae.tool import Corrupter, RankingLoss, display_info, get_date, load_dataset_of_embeddings, set_logging  # noqa: E402
from codae.train import HipEmbeddingTrainer, SubsetEpochSampler, fit_host_threads, shard_batch   # noqa: E402


def parse():
    p = argparse.ArgumentParser(description='Train denoising autoencoder.')
    p.add_argument('--embedding_path', type=str, required=True)
    p.add_argument('--output_path', type=str, required=True)
    p.add_argument('--config', type=str, required=True)
    p.add_argument('--debug', type=bool, default=False)
    p.add_argument('--rank', type=bool, default=False)
    p.add_argument('--nb_missing', type=int, default=1)
    p.add_argument('--precision', type=str, default=None, choices=[None, "bf16", "f32"])
    p.add_argument('--epochs', type=int, default=None)
    p.add_argument('--resume', type=str, default=None)
    return p.parse_args()


def main():
    args = parse()
    fit_host_threads()              # torch / BLAS pools no wider than the container's CPU quota (codae/train.py)
    log = set_logging(logging_level=(logging.DEBUG if args.debug else logging.INFO), log_file_path="log/")
    with open(args.config, 'r') as stream:
        config = yaml.safe_load(stream)
    mc, dc = config["MODEL"], config["DATASET"]

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise HipError("no HIP device: this build has no CPU path")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        import torch.distributed as dist
        from codae.train import init_rccl_process_group, seed_all_ranks
        init_rccl_process_group(device)
        # identical sampler order, Corrupter tables and initial weights on every rank (the reference seeds none of them)
        seed_all_ranks(int(config["SEED"]))

    log.info("Loading dataset.")
    # HIP: KEEP_INCOMPLETE: true (+ MIN_PRESENT: 2) (build-only keys): keep the observations that have at least MIN_PRESENT of
    # the used categories; their absent slots stay out of the input, the loss, the monitors and complete()'s inventory
    keep_incomplete = bool(config.get("HIP", {}).get("KEEP_INCOMPLETE", False))
    if keep_incomplete:
        dataset = load_dataset_of_embeddings(embedding_path=args.embedding_path, config=config, cache_dir="tmp/", keep_incomplete=True,
                                             min_present=int(config.get("HIP", {}).get("MIN_PRESENT", 2)))
        log.info("Keeping incomplete observations: %d of %d slots are absent" % (int((dataset.presence == 0).sum()), dataset.presence.size))
    else:
        dataset = load_dataset_of_embeddings(embedding_path=args.embedding_path, config=config, cache_dir="tmp/")
    dataset_std = torch.std(dataset.data)
    log.info("Dataset STD = " + str(dataset_std))
    log.info("CUDA available, loading GPU device")

    # split exactly as the reference (:102-116)
    indices = list(range(dataset.nb_observation))
    nb_train = math.floor(dataset.nb_observation * dc["SPLIT"][0])
    nb_validation = dataset.nb_observation - nb_train
    if dc["SHUFFLE"]:
        np.random.seed(config["SEED"])
        np.random.shuffle(indices)
    train_indices, validation_indices = indices[:nb_train], indices[nb_train:]
    # --resume: the split and (below) the mask table are the interrupted run's: this script seeds neither in a single process
    resumed = None
    if args.resume is not None:
        from codae.tool.checkpoint import read_checkpoint
        resumed = read_checkpoint(args.resume)[1]["extra"]
        if "epoch" not in resumed or "rng" not in resumed:
            raise HipError("--resume %s: not an epoch-boundary checkpoint of this script" % args.resume)
        train_indices, validation_indices = list(resumed["train_indices"]), list(resumed["validation_indices"])
        if len(train_indices) != nb_train or len(validation_indices) != nb_validation:
            raise HipError("--resume %s: the file's split is %d + %d rows, this dataset and config give %d + %d"
                           % (args.resume, len(train_indices), len(validation_indices), nb_train, nb_validation))
    train_sampler = SubsetEpochSampler(train_indices, mc["BATCH_SIZE"])
    validation_sampler = SubsetEpochSampler(validation_indices, mc["BATCH_SIZE"])

    # the reference draws an unused per-observation sample here; keep Python's RNG in step (:131-132)
    c = list(range(len(dc["USED_CATEGORY"])))
    [random.sample(c, len(c)) for _ in range(dataset.nb_observation)]
    corrupter = Corrupter(nb_observation=dataset.nb_observation, arch=dataset.arch, k_max=args.nb_missing, device=device)
    if resumed is not None:
        table = torch.tensor(resumed["mask_to_use"], dtype=torch.long)
        if table.shape != corrupter.mask_to_use.shape:
            raise HipError("--resume %s: the file's mask table is %s, this run's %s" % (args.resume, tuple(table.shape),
                                                                                      tuple(corrupter.mask_to_use.shape)))
        corrupter.mask_to_use = table
        corrupter.mask_to_use_i32 = table.to(torch.int32).contiguous().to(device)

    presence, mask_to_use = None, corrupter.mask_to_use_i32
    if keep_incomplete:
        from codae.tool import SlotPresence
        presence = SlotPresence(dataset.presence)
        # every row's runs reordered so that run 0 blanks a slot the row has and leaves one of its slots visible
        mask_to_use = presence.assign_masks(corrupter).to(device)

    log.info("Initializing the model.")
    io_size = dc["EMBEDDING_SIZE"] * len(dc["USED_CATEGORY"])
    if io_size % dc["EMBEDDING_SIZE"] != 0:
        raise Exception("Error: io_size must be a multiple of embedding_size")
    enc, dec = linear_stack(io_size, mc["Z_SIZE"], mc["NB_INPUT_LAYER"], mc["NB_OUTPUT_LAYER"], mc["STEEP_LAYER_SIZE"], False)
    precision = args.precision or config.get("HIP", {}).get("PRECISION", "bf16")
    # HIP: ACTIVATION: <torch.nn module name> (build-only key, like PRECISION): what follows each hidden Linear, built as
    # the model classes build it (activation(True)); absent = ReLU
    act_name = config.get("HIP", {}).get("ACTIVATION")
    activation = getattr(torch.nn, act_name) if act_name else None
    if act_name and not (isinstance(activation, type) and issubclass(activation, torch.nn.Module)):
        raise HipError("HIP: ACTIVATION: %r is not a torch.nn module" % act_name)
    dataset.to(device)
    # HIP: INPUT_NOISE: {KIND: gaussian | masking | salt_pepper, SIGMA | P: ..., LO: ..., HI: ..., SEED: ...} (build-only key):
    # noise on the training input in front of the slot blank; LO / HI default to the resident data's min / max.
    # {KIND: swap, P: 0.15, SEED: 7, POOL: train | all}: a slot replaced by another row's item of that slot; POOL: train (the default)
    # takes the items from the training rows only, so that no validation item ever reaches a training input
    from codae.tool.noise import input_noise_from_config
    input_noise = input_noise_from_config(config.get("HIP", {}).get("INPUT_NOISE"), dataset.data, train_rows=train_indices)
    if input_noise is not None and input_noise.kind == "swap":
        log.info("INPUT NOISE: swap, p = %g, pool of %d rows" % (input_noise.p, dataset.nb_observation if input_noise.pool is None
                                                                 else input_noise.pool.size))
    # HIP: LOSS_EMPHASIS: {ALPHA: ..., BETA: ..., SLOT_WEIGHT: [..] | COLUMN_WEIGHT: [..]} (build-only key): the training loss weights
    # corrupted elements by ALPHA, untouched ones by BETA, every slot / column by its weight (the monitors stay unweighted)
    from codae.tool.emphasis import loss_emphasis_from_config
    loss_emphasis = loss_emphasis_from_config(config.get("HIP", {}).get("LOSS_EMPHASIS"))
    # HIP: HIDDEN_DROPOUT: {P: 0.5 | [.. one per hidden output ..], SEED: ...} (build-only key): dropout on the output of every
    # hidden Linear of the training steps (validation never drops)
    from codae.tool.dropout import hidden_dropout_from_config
    hidden_dropout = hidden_dropout_from_config(config.get("HIP", {}).get("HIDDEN_DROPOUT"))
    # HIP: RESIDUAL: {LAYERS: hidden | [1, 2, ..]} (build-only key): an identity skip around the chosen hidden layers of equal widths,
    # in training and in validation alike (it is part of the model)
    from codae.tool.residual import residual_from_config
    residual = residual_from_config(config.get("HIP", {}).get("RESIDUAL"))
    # HIP: NORM: {KIND: layer | rms, LAYERS: hidden | [0, 1, ..], EPS: 1e-5} (build-only key): parameter-free normalisation of the chosen
    # layers' outputs per batch row, in training and in validation alike (it is part of the model)
    from codae.tool.norm import norm_from_config
    norm = norm_from_config(config.get("HIP", {}).get("NORM"))
    # HIP: SPARSE_CODE: {KEEP: 32, LAYER: null} (build-only key): the hard top-k code layer - the KEEP largest-magnitude units of the
    # code per row, in training and in validation alike (it is part of the model); LAYER null = the stack's code layer
    from codae.tool.sparse import sparse_from_config
    sparse_code = sparse_from_config(config.get("HIP", {}).get("SPARSE_CODE"))
    # HIP: CRITERION: {KIND: mse | l1 | smooth_l1 | huber | slot_cosine, BETA: .., DELTA: .., MSE_WEIGHT: ..} (build-only key): the
    # training loss instead of the mean squared error (the monitors stay squared-error sums; validation never sees it)
    from codae.tool.recon_loss import recon_loss_from_config
    criterion = recon_loss_from_config(config.get("HIP", {}).get("CRITERION"))
    # HIP: CONTRAST: {NEGATIVES: 256, TEMPERATURE: 0.1, WEIGHT: 1.0, SEED: 0, DISTINCT: true} (build-only key): a sampled softmax
    # over the true item of each slot and NEGATIVES rows drawn per step from the dataset, added to the criterion's loss
    from codae.tool.contrast import contrast_from_config
    contrast = contrast_from_config(config.get("HIP", {}).get("CONTRAST"))
    # HIP: OPTIMIZER: {KIND: adam | adamw | sgd | lamb | lars, AMSGRAD: false, MOMENTUM: 0.9, NESTEROV: true, TRUST_CLIP: 0,
    # TRUST_COEF: 0.001, DECAY_BIAS: false, SCHEDULE: {KIND: cosine, WARMUP: 100,
    # TOTAL: 10000, MIN_FACTOR: 0.01}} (build-only key): the update instead of Adam with L2 decay at a constant rate; a SCHEDULE
    # without TOTAL runs over this script's own loop: epochs x runs (one mask run) x batches per epoch
    from codae.tool.optimizer import optimizer_from_config
    epochs = args.epochs if args.epochs is not None else mc["EPOCH"]
    optimizer = optimizer_from_config(config.get("HIP", {}).get("OPTIMIZER"), total_steps=max(1, epochs * 1 * len(train_sampler)))

    # HIP: TIED_WEIGHTS: true (build-only key): the decoder's Linears use the transposed matrices of the encoder's (Vincent et al.
    # 2010); needs a mirror-symmetric stack (NB_INPUT_LAYER == NB_OUTPUT_LAYER)
    from codae.tool import TiedWeights
    tied_weights = TiedWeights.from_config(config.get("HIP", {}).get("TIED_WEIGHTS"))

    # HIP: WEIGHT_AVERAGE: {KIND: ema | swa, DECAY: 0.999, DEBIAS: true, START: 1 | START_EPOCH: k, EVERY: 1} (build-only key): the update
    # also keeps an average of the parameters it produces, and the validation sweep below runs on that average; START_EPOCH counts
    # this script's own batches per epoch
    from codae.tool.average import weight_average_from_config
    weight_average = weight_average_from_config(config.get("HIP", {}).get("WEIGHT_AVERAGE"), batches_per_epoch=max(1, len(train_sampler)))
    eval_weights = "average" if weight_average is not None and not weight_average.is_default else "live"

    def build(prec):
        return HipEmbeddingTrainer(enc + dec, dataset.data, corrupter.mask_table_u8, mask_to_use,
                                   mc["LEARNING_RATE"], mc["WEIGHT_DECAY"], clip=1.0 if mc["TRUNK_GRAD"] else 0.0,
                                   max_batch=mc["BATCH_SIZE"], precision=prec, device=device, distributed=world > 1,
                                   activation=activation, input_noise=input_noise, loss_emphasis=loss_emphasis,
                                   hidden_dropout=hidden_dropout, criterion=criterion, contrast=contrast, optimizer=optimizer,
                                   presence=presence, tied_weights=tied_weights, weight_average=weight_average, residual=residual, norm=norm,
                                   sparse_code=sparse_code)
    try:
        trainer = build(precision)
    except HipError as e:
        if precision != "bf16":
            raise
        log.info("bf16 tiles cannot take this stack (%s): using the exact-fp32 kernels" % e)
        trainer = build("f32")
    trainer.init_params(seed=int(torch.empty((), dtype=torch.int64).random_().item()) % (2 ** 31))

    display_info(config, dataset.nb_observation, {})
    act_label = "+" + (activation(True).__class__.__name__ if activation is not None else "ReLU")
    log.info("Linear stack: " + " | ".join("%d->%d%s" % (k, n, act_label if r else "") for k, n, r in enc + dec))
    if tied_weights:
        log.info("TIED WEIGHTS: %d free parameters of %d" % (TiedWeights.free_parameter_count(enc + dec),
                                                            sum(k * n + n for k, n, _ in enc + dec)))
    if trainer.engine.residual_layers:
        log.info("RESIDUAL: %r - identity skips around layers %s" % (residual, trainer.engine.residual_layers))
    if trainer.engine.norm_layers:
        log.info("NORM: %r - %s normalisation of the outputs of layers %s" % (norm, norm.kind, trainer.engine.norm_layers))
    if trainer.engine.sparse_resolved is not None:
        log.info("SPARSE CODE: keep %d of %d at layer %d" % (sparse_code.keep, trainer.engine.sparse_resolved[1], trainer.engine.sparse_resolved[0] + 1))
    if eval_weights == "average":
        log.info("WEIGHT AVERAGE: %r - the validation errors and the ranking error are those of the averaged weights" % (weight_average,))
    book = {k: [] for k in ("ftl", "ptl", "fvl", "pvl", "rl")}
    S = dataset.nb_used_category
    rank_indices, nb_ranked = validation_indices, nb_validation
    if keep_incomplete:
        # the four RMSE monitors divide by what the sums ran over (SlotPresence.counts, in slots: times E = elements); the
        # ranking monitor sees the complete validation rows only (its inventory has no notion of an absent item)
        E = dataset.embedding_size
        m2u_host = mask_to_use.cpu()
        den = {}
        for name, rows in (("train", train_indices), ("validation", validation_indices)):
            full, part = presence.counts(rows, mask_ids=m2u_host[torch.as_tensor(rows, dtype=torch.long), 0], mask_table=corrupter.binary_masks)
            den[name] = (max(full, 1) * E, max(part, 1) * E)
        complete_row = dataset.presence.all(axis=1)
        rank_indices = [i for i in validation_indices if complete_row[i]]
        nb_ranked = max(len(rank_indices), 1)
    else:
        den = {"train": (dataset.nb_predictor * nb_train, nb_train * dataset.nb_predictor / S),
               "validation": (dataset.nb_predictor * nb_validation, nb_validation * dataset.nb_predictor / S)}
    ranking_loss = RankingLoss(dataset, rank_indices if rank_indices else validation_indices, device=device)
    is_ranked = None
    if keep_incomplete:
        is_ranked = torch.zeros(dataset.nb_observation, dtype=torch.bool, device=device)
        if rank_indices:
            is_ranked[torch.as_tensor(rank_indices, dtype=torch.long, device=device)] = True
    # HIP: RETRIEVAL_METRICS: {K: [1, 10, 50], DISTINCT: true} (build-only key): hit@k and MRR of every blanked slot of EVERY
    # validation row - the incomplete ones included, each ranked among the validation rows that have the slot - beside the ranking
    # error; absent = nothing is added to the sweep, the log or book.json
    from codae.tool import retrieval_metrics_from_config
    rm_args = retrieval_metrics_from_config(config.get("HIP", {}).get("RETRIEVAL_METRICS"))
    retrieval = trainer.retrieval_metrics(validation_indices, **rm_args) if rm_args is not None else None
    if retrieval is not None:
        book.update({k: [] for k in ["mrr"] + ["hit@%d" % k for k in retrieval.ks] + ["ranked_pairs"]})
    # HIP: COMPATIBILITY: {NEGATIVES: 1, SEED: 0, DISTINCT: true} (build-only key): compatibility prediction on the validation rows -
    # every row scored as an outfit (each item left out in turn and reconstructed from the others) against NEGATIVES copies of it with
    # one item swapped for another validation row's: the AUC and the share of swapped outfits that score below their original;
    # absent = nothing is added to the sweep, the log or book.json
    from codae.tool import compatibility_from_config
    cm_args = compatibility_from_config(config.get("HIP", {}).get("COMPATIBILITY"))
    compat = trainer.compatibility_metrics(validation_indices, **cm_args) if cm_args is not None else None
    if compat is not None:
        book.update({k: [] for k in ("auc", "paired_acc", "scored_outfits")})

    # HIP: CHECKPOINT: {EVERY: 1, KEEP: 2, DIR: ...} (build-only key): a checkpoint file after every EVERY-th epoch's validation sweep,
    # the newest KEEP kept; absent (and no --resume) = nothing is logged, written or drawn differently
    ck = config.get("HIP", {}).get("CHECKPOINT")
    ck_every = ck_keep = 0
    if ck is not None:
        unknown = set(ck) - {"EVERY", "KEEP", "DIR"}
        if unknown:
            raise HipError("HIP: CHECKPOINT: unknown keys %s" % sorted(unknown))
        ck_every, ck_keep = int(ck.get("EVERY", 1)), int(ck.get("KEEP", 2))
        if ck_every < 1 or ck_keep < 1:
            raise HipError("HIP: CHECKPOINT: EVERY and KEEP must be at least 1, got %d and %d" % (ck_every, ck_keep))
    # HIP: CODES: {SAVE: true, LAYER: null, NEIGHBOURS: 0, DISTINCT: true} (build-only key): after the last epoch every dataset row is
    # encoded - on the averaged weights when WEIGHT_AVERAGE is set, as the validation sweep - and codes.npz goes to the run directory:
    # codes [N, Z], rows, layer and, with NEIGHBOURS k > 0, each row's k nearest other rows in code space; absent = nothing is encoded,
    # logged or written
    from codae.tool import codes_from_config
    codes_cfg = codes_from_config(config.get("HIP", {}).get("CODES"))
    # HIP: CODE_CLUSTERS: {K: 64, ITERS: 25, SEED: 0, LAYER: null} (build-only key): after the last epoch the codes of every dataset row
    # - those CODES encoded when both keys name the same layer - are clustered by spherical k-means and clusters.npz goes to the run
    # directory: centroids, cluster [N], score [N], counts, objective, changed, rows, layer; absent = nothing is encoded, logged or written
    from codae.tool import clusters_from_config
    clusters_cfg = clusters_from_config(config.get("HIP", {}).get("CODE_CLUSTERS"))
    run_dir = []

    def out_dir():
        if not run_dir:
            run_dir.append(os.path.join(args.output_path, get_date() + "_train_" + dc["NAME"]))
            os.makedirs(run_dir[0], exist_ok=True)
        return run_dir[0]

    from codae.tool.checkpoint import StateDigest
    data_digest = StateDigest.hex(trainer.engine.digest(trainer.data)) if (ck is not None or resumed is not None) else None
    first_epoch = 0
    if resumed is not None:
        if resumed["dataset_digest"] != data_digest:
            raise HipError("--resume %s: the file was written over a dataset with digest %s, this run's dataset has %s"
                           % (args.resume, resumed["dataset_digest"], data_digest))
        trainer.load(args.resume)
        for k, v in resumed["book"].items():
            book[k] = list(v)
        first_epoch = int(resumed["epoch"])
        rng = resumed["rng"]
        torch.set_rng_state(torch.tensor(rng["torch"], dtype=torch.uint8))
        np.random.set_state((rng["numpy"][0], np.asarray(rng["numpy"][1], dtype=np.uint32), rng["numpy"][2], rng["numpy"][3], rng["numpy"][4]))
        random.setstate((rng["python"][0], tuple(rng["python"][1]), rng["python"][2]))
        log.info("RESUMED %s: %d epochs done, state digest %s" % (args.resume, first_epoch, StateDigest.hex(trainer.state_digest()["all"])))
    pending, written = [], []

    def write_pending():
        # the file write hides behind the device work enqueued since the snapshot
        while pending:
            snap, path, extra = pending.pop()
            all_digest = StateDigest.hex(StateDigest.combine(snap.digests().values()))
            nbytes = snap.write(path, extra=extra)
            log.info("CHECKPOINT %s: %d bytes, state digest %s" % (path, nbytes, all_digest))
            written.append(path)
            while len(written) > ck_keep:
                old = written.pop(0)
                if os.path.exists(old):
                    os.remove(old)

    for epoch in range(first_epoch, epochs):
        log.info("===================================================== EPOCH = %d" % epoch)
        if optimizer is not None:
            log.info("LEARNING RATE            = %.6g" % trainer.current_lr())
            if getattr(optimizer, "is_trust", False) and trainer.engine.step_count > 0:
                # lamb / lars: the layer-wise ratios of the last update (one read of a few floats per epoch)
                lo, hi = (float(x) for x in torch.aminmax(trainer.trust_ratios()))
                log.info("TRUST RATIO min / max    = %.6g / %.6g" % (lo, hi))
        for batch_indices in train_sampler.device_batches(device):      # one index copy per epoch, int32, on the device
            shard = shard_batch(batch_indices, rank, world)
            if shard is None:                   # fewer rows than ranks (ragged last batch): skipped by every rank
                nb_skipped = len(batch_indices)
                log.info("skipping a global batch of %d rows on %d ranks" % (nb_skipped, world))
                continue
            trainer.train_batch(shard.contiguous(), run=0, global_rows=len(batch_indices))
            if pending:
                write_pending()
        sq, sqp = trainer.epoch_sums()
        book["ftl"].append(np.sqrt(sq / den["train"][0]))
        book["ptl"].append(np.sqrt(sqp / den["train"][1]))
        log.info("TRAINING FULL ERROR      = %7f" % book["ftl"][-1])
        log.info("TRAINING PARTIAL ERROR   = %7f" % book["ptl"][-1])

        # validation (reference :241-261) stays on the device: forward + metric sums in the engine, the rank metric as
        # batched GEMMs against the validation inventory with the masks taken from the Corrupter's device tables; one
        # read-back per epoch instead of a mask expansion, two .tolist() and a host sync per batch
        for idx in validation_sampler.device_batches(device):
            y = trainer.eval_batch(idx, run=0, want_y=True, weights=eval_weights)
            if is_ranked is None:
                ranking_loss.add(y, idx, corrupter, run=0)
            elif rank_indices:
                keep = is_ranked[idx.long()]
                if bool(keep.any()):
                    ranking_loss.add(y[keep].contiguous(), idx[keep].contiguous(), corrupter, run=0)
            if retrieval is not None:
                retrieval.add(y, idx, run=0)
            if compat is not None:
                compat.add_batch(idx, weights=eval_weights)
        rl = ranking_loss.total() if (is_ranked is None or rank_indices) else 0.0     # (no complete validation row: nothing was ranked)
        sq, sqp = trainer.epoch_sums(reduce=False)      # every rank evaluates the whole validation set
        book["fvl"].append(np.sqrt(sq / den["validation"][0]))
        book["pvl"].append(np.sqrt(sqp / den["validation"][1]))
        book["rl"].append(rl / nb_ranked)
        log.info("VALIDATION FULL ERROR    = %7f" % book["fvl"][-1])
        log.info("VALIDATION PARTIAL ERROR = %7f" % book["pvl"][-1])
        log.info("VALIDATION RANKING ERROR = %7f" % book["rl"][-1])
        if retrieval is not None:
            rm = retrieval.total()
            for k in retrieval.ks:
                book["hit@%d" % k].append(rm["hit@%d" % k])
                log.info("VALIDATION HIT@%-4d       = %7f" % (k, rm["hit@%d" % k]))
            book["mrr"].append(rm["mrr"])
            book["ranked_pairs"].append(rm["pairs"])
            log.info("VALIDATION MRR           = %7f" % rm["mrr"])
            log.info("VALIDATION RANKED PAIRS  = %d" % rm["pairs"])
        if compat is not None:
            cm = compat.total()
            book["auc"].append(cm["auc"])
            book["paired_acc"].append(cm["paired_acc"])
            book["scored_outfits"].append(cm["outfits"])
            log.info("VALIDATION COMPATIBILITY AUC = %7f" % cm["auc"])
            log.info("VALIDATION PAIRED ACCURACY   = %7f" % cm["paired_acc"])
            log.info("VALIDATION SCORED OUTFITS    = %d" % cm["outfits"])
        write_pending()                  # (an epoch that trained no batch)
        if ck is not None and rank == 0 and (epoch + 1) % ck_every == 0:
            # two phases: the snapshot here, at the epoch boundary; the file once the next epoch's first batch is enqueued (or at exit)
            np_state, py_state = np.random.get_state(), random.getstate()
            extra = {"epoch": epoch + 1, "book": {k: [float(v) for v in vs] for k, vs in book.items()},
                     "train_indices": [int(i) for i in train_indices], "validation_indices": [int(i) for i in validation_indices],
                     "mask_to_use": corrupter.mask_to_use.tolist(), "dataset_digest": data_digest,
                     "rng": {"torch": torch.get_rng_state().tolist(),
                             "numpy": [np_state[0], np_state[1].tolist(), int(np_state[2]), int(np_state[3]), float(np_state[4])],
                             "python": [py_state[0], list(py_state[1]), py_state[2]]}}
            ck_dir = ck.get("DIR") or out_dir()
            os.makedirs(ck_dir, exist_ok=True)
            pending.append((trainer.snapshot(), os.path.join(ck_dir, "checkpoint_epoch%d.npz" % (epoch + 1)), extra))
    write_pending()
    log.info("TRAINING HAS ENDED.")

    index = None
    if codes_cfg is not None and rank == 0:
        index = trainer.code_index(layer=codes_cfg["layer"], weights=eval_weights, distinct=codes_cfg["distinct"])
        n_rows = len(index)
        out = {"codes": index.bank.cpu().numpy(), "rows": np.arange(n_rows, dtype=np.int64), "layer": np.int64(index.layer)}
        if codes_cfg["neighbours"] > 0:
            nb_idx, nb_score = [], []
            for o in range(0, n_rows, trainer.engine.max_batch):          # self excluded: neighbours other than the outfit itself
                rows = torch.arange(o, min(o + trainer.engine.max_batch, n_rows), device=device)
                i, s = index.similar(index.bank[rows], codes_cfg["neighbours"], exclude=rows)
                nb_idx.append(i.cpu().numpy()); nb_score.append(s.cpu().numpy())
            out["neighbour_idx"], out["neighbour_score"] = np.concatenate(nb_idx), np.concatenate(nb_score)
        codes_path = os.path.join(out_dir(), "codes.npz")
        np.savez(codes_path, **out)
        log.info("OUTFIT CODES: [%d, %d] layer %d -> %s" % (n_rows, index.width, index.layer, codes_path))

    if clusters_cfg is not None and rank == 0:
        want = trainer.code_layers if clusters_cfg["layer"] is None else clusters_cfg["layer"]
        reused = index is not None and index.layer == want                    # CODES encoded this layer already: one bank for both files
        if not reused:
            index = trainer.code_index(layer=clusters_cfg["layer"], weights=eval_weights)
        fit = index.cluster(clusters_cfg["k"], iters=clusters_cfg["iters"], seed=clusters_cfg["seed"])
        counts = fit.counts.cpu().numpy()
        objective = fit.objective.cpu().numpy()
        clusters_path = os.path.join(out_dir(), "clusters.npz")
        np.savez(clusters_path, centroids=fit.centroids.cpu().numpy(), cluster=fit.assign.cpu().numpy(), score=fit.score.cpu().numpy(),
                 counts=counts, objective=objective, changed=fit.changed.cpu().numpy(), rows=np.arange(len(index), dtype=np.int64),
                 layer=np.int64(index.layer))
        log.info("OUTFIT CLUSTERS: K %d, %d iterations, converged_at %s, objective %.6f, %d empty, bank %s -> %s" % (
            fit.k, clusters_cfg["iters"], fit.converged_at, float(objective[-1]), int((counts == 0).sum()),
            "reused" if reused else "encoded", clusters_path))

    if rank == 0:
        import matplotlib
        matplotlib.use('agg')
        import matplotlib.pyplot as plt
        d = out_dir()
        axis = np.arange(0, epochs)
        for name, a, b, extra in (("full_RMSE", "ftl", "fvl", None), ("partial_RMSE", "ptl", "pvl", float(dataset_std))):
            plt.plot(axis, book[a], label="Training")
            plt.plot(axis, book[b], label="Validation")
            if extra is not None:
                plt.plot(axis, [extra] * len(axis), label="Validation standard deviation")
            plt.xlabel('Epoch'); plt.ylabel('RMSE'); plt.legend(loc='best')
            plt.savefig(os.path.join(d, name + ".png")); plt.clf()
        if args.rank:
            plt.plot(axis, book["rl"], label="RIRE"); plt.plot(axis, [0.5] * len(axis), label="Random rank")
            plt.xlabel('Epoch'); plt.ylabel('RIRE'); plt.legend(loc='best')
            plt.savefig(os.path.join(d, "partial_RIRE.png")); plt.clf()
        with open(os.path.join(d, "book.json"), "w") as f:
            import json
            json.dump({k: [float(v) for v in vs] for k, vs in book.items()}, f)
        log.info("Data saved in directory %s" % d)
    return book


if __name__ == "__main__":
    main()
