"""03b_irn/step/train_irn.py on libwsscam: IRNet training from image and IR-label files to a saved state dict.

run(args) takes the reference's argument names (train_irn.py:14-168):
    irn_network, model_dir, dataset, tag, num_classes, use_cls     the model (step.make_sem_seg_labels._build_model)
    irn_crop_size, irn_batch_size, irn_num_epoches, irn_learning_rate, irn_weight_decay
    train_list, infer_list, ir_label_out_dir, dev_root, crop_method, rescale_range, outsize, norm_mode
    irn_weights_name                                               where IrnTrainer.save writes
    num_workers                                                    decode threads (default 8; never the machine's CPU count)
and, beyond the reference's: state_dict (the initial EdgeDisplacement state dict -- the reference builds it from the CAM
checkpoint under model_dir and torch's random head initialisation, neither of which is here; or irn_init_weights_name, a file
np.save'd from such a dict), seed (the epoch shuffles; None: unseeded), irn_precision, irn_path_radius (the reference's constant
10; a crop below 80 leaves no pair inside it).

Per step: decode (PIL, on the thread pool, one batch prefetched) -> the draws of the batch's records in sample order (Python's
`random`, the reference's order) -> irn_train.TrainBatcher.apply (wsc_irn_train_batch) -> IrnTrainer.step.  The three dataset
branches, the shuffled order per epoch with drop_last, max_step, the progress line every 50 steps and the closing pass over the
infer list (top-left crop, 'int' normalisation, drop_last) through IrnTrainer.fit_dp_mean follow the reference.  DataParallel is
out of scope: one device."""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .. import irn_train
from ..misc import indexing
from ..misc.imutils import prefetched as _prefetched
from .make_sem_seg_labels import _build_model


def build_datasets(args):
    """-> (train dataset, infer dataset): train_irn.py:22-79"""
    common = dict(label_dir=args.ir_label_out_dir, dev_root=args.dev_root, hor_flip=True, crop_size=args.irn_crop_size,
                  crop_method=args.crop_method, rescale=args.rescale_range, outsize=args.outsize, norm_mode=args.norm_mode)
    if args.dataset == "voc12":
        from ..voc12 import dataloader as dl

        return dl.VOC12AffinityDataset(args.train_list, **common), dl.VOC12ImageDataset(args.infer_list, dev_root=args.dev_root)
    if args.dataset in ("adp_morph", "adp_func"):
        from ..adp import dataloader as dl

        htt = args.dataset.split("_")[-1]
        return (dl.ADPAffinityDataset(args.train_list, is_eval=args.dataset == "evaluation", htt_type=htt, **common),
                dl.ADPImageDataset(args.infer_list, dev_root=args.dev_root, htt_type=htt, is_eval=args.dataset == "evaluation"))
    if args.dataset in ("deepglobe", "deepglobe_balanced"):
        from ..deepglobe import dataloader as dl

        bal = args.dataset == "deepglobe_balanced"
        return (dl.DeepGlobeAffinityDataset(args.train_list, is_balanced=bal, **common),
                dl.DeepGlobeImageDataset(args.infer_list, dev_root=args.dev_root, is_balanced=bal))
    raise KeyError("Dataset %s not yet implemented" % args.dataset)


def _initial_state_dict(args):
    if getattr(args, "state_dict", None) is not None:
        return args.state_dict
    name = getattr(args, "irn_init_weights_name", None)
    if not name:
        raise ValueError("train_irn.run: args.state_dict (or args.irn_init_weights_name) must give the initial EdgeDisplacement state dict")
    return irn_train.IrnTrainer._read(name)[0]


def _infer_batches(pool, batcher, infer_dataset, bs):
    """the closing pass's inputs: the infer list in order, drop_last, each batch one float32 DeviceMaps (B, 3, S, S) that lives
    until the consumer asks for the next one (train_irn.py:35-38, 148-158: top-left crop, 'int' normalisation)"""
    S = batcher.crop_size
    n = len(infer_dataset) // bs
    for _, packs in _prefetched(pool, (range(k * bs, (k + 1) * bs) for k in range(n)), lambda i: infer_dataset[i]["img"]):
        params = [(im.shape[0], im.shape[1], 0, 0, 0, 0, 0, min(S, im.shape[0]), min(S, im.shape[1])) for im in packs]
        x, label, reduced = batcher.apply(packs, [np.zeros(im.shape[:2], np.uint8) for im in packs], np.array(params, np.int32))
        label.free()
        reduced.free()
        try:
            yield x
        finally:
            x.free()


def run(args):
    S, bs = int(args.irn_crop_size), int(args.irn_batch_size)
    # (train_irn.py:16: radius 10; the host index arrays of default_size are not built: the pair labels are formed on the device)
    path_index = indexing.PathIndex(radius=getattr(args, "irn_path_radius", None) or 10)
    train_dataset, infer_dataset = build_datasets(args)
    model = _build_model(args)
    model.load_state_dict(_initial_state_dict(args), strict=False)
    model.eval().cuda(int(getattr(args, "device", 0) or 0))
    ctx = model.ctx
    steps_per_epoch = len(train_dataset) // bs
    max_step = steps_per_epoch * int(args.irn_num_epoches)
    if max_step < 1:
        raise ValueError("train_irn.run: %d training samples give no batch of %d" % (len(train_dataset), bs))
    batcher = irn_train.TrainBatcher(ctx, S, args.norm_mode, outsize=args.outsize, normalize=train_dataset.normalize_cls,
                                     rescale=args.rescale_range)
    rng = np.random.default_rng(getattr(args, "seed", None))
    n_threads = max(1, int(getattr(args, "num_workers", None) or 8))
    sums, count = np.zeros(4), 0
    t_start = time.time()
    with irn_train.IrnTrainer(model, path_index, args.irn_learning_rate, args.irn_weight_decay, max_step) as trainer, \
            ThreadPoolExecutor(max_workers=n_threads) as pool:
        for ep in range(int(args.irn_num_epoches)):
            print("Epoch %d/%d" % (ep + 1, args.irn_num_epoches))
            order = rng.permutation(len(train_dataset))  # DataLoader(shuffle=True, drop_last=True)
            t_stage = time.time()
            epoch = (order[k * bs:(k + 1) * bs] for k in range(steps_per_epoch))
            for it, (idxs, decoded) in enumerate(_prefetched(pool, epoch, train_dataset.decoded)):
                params = np.stack([train_dataset.draw(int(i), d[0].shape[:2]) for i, d in zip(idxs, decoded)])
                lr_now = trainer.lr[0]
                x, label, reduced = batcher.apply([d[0] for d in decoded], [d[1] for d in decoded], params)
                with x, label, reduced:
                    losses = trainer.step(x, reduced)
                sums += (losses["pos"], losses["neg"], losses["dp_fg"], losses["dp_bg"])
                count += 1
                if (trainer.global_step - 1) % 50 == 0:
                    done = trainer.global_step / max_step
                    eta = time.ctime(t_start + (time.time() - t_start) / done)
                    avg = sums / count
                    sums, count = np.zeros(4), 0
                    print("step:%5d/%5d" % (trainer.global_step - 1, max_step), "loss:%.4f %.4f %.4f %.4f" % tuple(avg),
                          "imps:%.1f" % ((it + 1) * bs / max(time.time() - t_stage, 1e-9)), "lr: %.4f" % lr_now, "etc:%s" % eta, flush=True)
        print("Analyzing displacements mean ... ", end="")
        n_infer = len(infer_dataset) // bs
        if n_infer < 1:
            raise ValueError("train_irn.run: %d infer samples give no batch of %d" % (len(infer_dataset), bs))
        infer_batcher = irn_train.TrainBatcher(ctx, S, "int", normalize=train_dataset.normalize_cls)
        model._ensure_net().set_mean_shift(np.zeros(2, np.float32))  # a freshly trained model: running_mean is zeros
        trainer.fit_dp_mean(_infer_batches(pool, infer_batcher, infer_dataset, bs), n_batches=n_infer)
        print("done.")
        trainer.save(args.irn_weights_name)
    return model
