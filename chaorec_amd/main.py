"""Entry point: `python -m chaorec_amd.main --Model LightGCN --data_path sports` (reference main.py:73-442).

Same flow: parse flags, seed, load data, build the sampler, cartesian product over the model's YAML grid,
construct the model, Adam, train_and_evaluate, keep the best combination by Recall@20.  Out of scope and
dropped: the 51 other constructors and the dense U x I DiffusionData the reference builds for every model
(main.py:202; 1.76 GB for sports)."""
import logging
import os
from itertools import product

import torch
from torch.utils.data import DataLoader

from . import dataload
from .arg_parser import load_yaml_config, parse_args
from .optim import FusedAdam
from .registry import MODELS, ModelData, spec_of
from .train_and_evaluate import train_and_evaluate
from .utils import get_local_time, gpu, setup_seed


def setup_logging(args):
    log_dir = "log"
    os.makedirs(log_dir, exist_ok=True)
    log_filename = os.path.join(log_dir, f"{args.Model}_{args.data_path}").replace("\\", "/") + ".log"
    fmt = logging.Formatter('%(asctime)s %(levelname)s %(message)s', '%a %d %b %Y %H:%M:%S')
    logger = logging.getLogger()
    logger.setLevel(logging.INFO)
    for h in (logging.StreamHandler(), logging.FileHandler(log_filename, mode='w')):
        h.setLevel(logging.INFO)
        h.setFormatter(fmt)
        logger.addHandler(h)


def build_model(args, num_user, num_item, train_data, user_item_dict, v_feat, t_feat, device):
    """The model's row of the constructor table (registry.MODELS), called with the flags and the loaded data."""
    if args.Model not in MODELS:
        raise SystemExit(f"--Model {args.Model}: only {sorted(MODELS)} are on the MI355X hot path")
    return MODELS[args.Model].build(args, ModelData(num_user, num_item, train_data, user_item_dict, v_feat, t_feat, device))


def main(argv=None):
    args = parse_args(argv)
    setup_logging(args)
    logging.info('============Arguments==============')
    for arg, value in vars(args).items():
        logging.info('%s: %s', arg, value)
    logging.info('local time：%s', get_local_time())
    setup_seed(args.seed)
    device = gpu()
    if device.type != "cuda":
        raise SystemExit("chaorec_amd runs on the MI355X only: no GPU visible")
    config = load_yaml_config(args.Model)
    spec = spec_of(args.Model)
    train_data, val_data, test_data, user_item_dict, num_user, num_item, v_feat, t_feat = dataload.data_load(
        args.data_path, has_v=spec.features, has_t=spec.features, data_root=args.data_root, synthetic=args.synthetic)
    if args.host_sampler:
        ds = dataload.TrainingDataset(num_user, num_item, user_item_dict, train_data, args.Model)
        train_loader = DataLoader(ds, args.batch_size, shuffle=True, num_workers=args.num_workers)
    else:
        train_loader = dataload.DeviceBatchSampler(num_user, num_item, user_item_dict, train_data, args.batch_size,
                                                   device, args.Model, args.seed)
    args.num_user, args.num_item = num_user, num_item

    combinators = list(product(*[config[p] for p in config['hyper_parameters']]))
    best_performance, best_params, best_metrics = None, None, None
    for idx, combo in enumerate(combinators):
        hyper = dict(zip(config['hyper_parameters'], combo))
        logging.info('========={}/{}: Parameters:{}========='.format(idx + 1, len(combinators), hyper))
        for key, value in hyper.items():
            setattr(args, key, value)
        model = build_model(args, num_user, num_item, train_data, user_item_dict, v_feat, t_feat, device)
        model.to(device)
        # reference: torch.optim.Adam (main.py:397); same update, one fused launch per tensor
        # (BSPM has no parameter: no optimizer, as its branch of train_and_evaluate never steps one; CF_Diff's epoch creates its
        # own AdamW over CAM_AE, train_and_evaluate.py:317)
        optimizer = FusedAdam([{'params': model.parameters(), 'lr': args.learning_rate}]) if spec.main_optimizer else None
        current = train_and_evaluate(model, train_loader, val_data, test_data, optimizer, args.num_epoch,
                                     model_name=args.Model, topk=args.topk, patience=args.patience,
                                     graph=not args.no_graph)
        recall = current[20]['recall'] if 20 in current else current[max(current)]['recall']
        if best_performance is None or recall > best_performance:
            best_performance, best_params, best_metrics = recall, hyper.copy(), current
    logging.info("Best performance: {:.5f}".format(best_performance))
    logging.info("Best parameters: {}".format(best_params))
    logging.info("Best metrics:")
    for k, m in best_metrics.items():
        logging.info(f"{k}: {' | '.join(f'{name}: {value:.5f}' for name, value in m.items())}")
    return best_metrics


if __name__ == '__main__':
    main()
