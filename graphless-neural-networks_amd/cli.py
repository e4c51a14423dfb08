"""Command-line surface of the reference's two entry points, kept flag-for-flag:
`train_teacher.py` (reference train_teacher.py:21-149, run :152-314) and `train_student.py`
(reference train_student.py:22-165, run :168-384).  Same flags and defaults, same YAML-overrides-CLI merge
(`conf = dict(args.__dict__, **conf)`, train_teacher.py:225-229), same output directory layout and artefacts
(out.npz = log-probs of ALL nodes, loss_and_score.npz, model.pth, min_cut_loss, exp_results).

The flag tables below are data; both parsers are built from them."""
import argparse
from pathlib import Path

import numpy as np
import torch
import yaml
from torch import optim

from .dataloader import load_data, load_out_t
from .kinds import BY_KIND, teacher_kind, teacher_names
from .models import Model
from .train_and_eval import distill_run_inductive, distill_run_transductive, run_inductive, run_transductive
from .utils import (check_readable, check_writable, compute_min_cut_loss, feature_prop, get_evaluator, get_logger,
                    get_training_config, graph_split, set_seed)

_DEFAULT_CONF = str(Path(__file__).resolve().parent.parent.joinpath("train.conf.yaml"))

# (flag, type-or-"store_true", default, help)
_COMMON = [
    ("device", int, -1, "CUDA device, -1 means CPU"), ("seed", int, 0, "Random seed"),
    ("log_level", int, 20, "Logger levels for run {10: DEBUG, 20: INFO, 30: WARNING}"),
    ("console_log", "store_true", False, "Set to True to display log info in console"),
    ("output_path", str, "outputs", "Path to save outputs"), ("num_exp", int, 1, "Repeat how many experiments"),
    ("exp_setting", str, "tran", "Experiment setting, one of [tran, ind]"),
    ("eval_interval", int, 1, "Evaluate once per how many epochs"),
    ("save_results", "store_true", False, "Save the loss curves, trained model, and min-cut loss"),
    ("dataset", str, "cora", "Dataset"), ("data_path", str, "./data", "Path to data"),
    ("labelrate_train", int, 20, "How many labeled data per class as train set"),
    ("labelrate_val", int, 30, "How many labeled data per class in valid set"),
    ("split_idx", int, 0, "For Non-Homo datasets only, one of [0,1,2,3,4]"),
    ("model_config_path", str, _DEFAULT_CONF, "Path to model configuration"),
    ("teacher", str, "SAGE", "Teacher model"), ("num_layers", int, 2, "Model number of layers"),
    ("hidden_dim", int, 128, "Model hidden layer dimensions"), ("dropout_ratio", float, 0, ""),
    ("norm_type", str, "none", "One of [none, batch, layer]"), ("batch_size", int, 512, ""),
    ("fan_out", str, "5,5", "Number of samples for each layer in SAGE. Length = num_layers"),
    ("num_workers", int, 0, "Number of workers for sampler"), ("learning_rate", float, 0.01, ""),
    ("weight_decay", float, 0.0005, ""), ("max_epoch", int, 500, "Maximum number of epochs"),
    ("patience", int, 50, "Early stop if the validation score does not improve for this many epochs"),
    ("feature_noise", float, 0, "add white noise to features for analysis, value in [0, 1]"),
    ("split_rate", float, 0.2, "Rate for graph split, see graph_split"),
    ("compute_min_cut", "store_true", False, "Compute and store the min-cut loss"),
    ("feature_aug_k", int, 0, "Augment node features by aggregating feature_aug_k-hop neighbour features"),
]
_STUDENT_ONLY = [
    ("student", str, "MLP", "Student model"),
    ("lamb", float, 0, "Parameter balancing hard-label loss (lamb) and teacher soft-label loss (1-lamb), in [0, 1]"),
    ("out_t_path", str, "outputs", "Path to load teacher outputs"),
]


def _parser(rows, description):
    p = argparse.ArgumentParser(description=description)
    for name, typ, default, hlp in rows:
        if typ == "store_true":
            p.add_argument(f"--{name}", action="store_true", help=hlp)
        else:
            p.add_argument(f"--{name}", type=typ, default=default, help=hlp)
    return p


def get_teacher_args(argv=None):
    p = _parser(_COMMON, "GLNN teacher (HIP hot path)")
    # not a reference flag: the activation storage of the SAGE teacher's whole-graph evaluation forward (Model.inference(dtype=...)),
    # bfloat16 = the gathered matrices stored as bf16, int8 = as int8 rows with one fp32 scale per row (docs/INT8_INFERENCE_SEMANTICS.md);
    # arithmetic and the saved log-probs fp32
    p.add_argument("--inference_dtype", type=str, default="float32", choices=["float32", "bfloat16", "int8"],
                   help="Activation storage of the SAGE teacher's evaluation forward (bfloat16, int8: SAGE only)")
    # not a reference flag: neighbour-sampled evaluation of the SAGE teacher (conf key `inference_fan_out`, read by run_transductive /
    # run_inductive; docs/SAMPLED_INFERENCE_SEMANTICS.md): every evaluation forward aggregates at most this many uniformly drawn in-edges
    # per row and layer, drawn under --seed.  Empty (the default) = off: the full-neighbour forward
    p.add_argument("--inference_fan_out", type=str, default="",
                   help="Per-layer fan-out of the SAGE teacher's evaluation forwards, e.g. 15,15 (length = --num_layers, values in [1, 64]; "
                        "empty: full-neighbour)")
    # not a reference flag: the SAGE teacher's aggregator (conf key `sage_aggregator`, read by Model): "gcn" is what the reference builds,
    # "mean" dgl's default form with a separate fc_self (docs/SAGE_MEAN_SEMANTICS.md; trained through the differentiable ops, fp32 inference)
    p.add_argument("--sage_aggregator", type=str, default="gcn", choices=["gcn", "mean"],
                   help="Aggregator of the SAGE teacher's SAGEConv layers (mean: separate fc_self; fp32, single device)")
    # not a reference flag: how a SAGE "mean" teacher steps (train_sage(mean_step=...)): "autograd" = the differentiable ops + torch's loss and
    # optimiser, "native" = TeacherEngine.step_sage_mean, the whole step as one C call (csrc/sage_mean_step.hip)
    p.add_argument("--sage_mean_step", type=str, default="autograd", choices=["autograd", "native"],
                   help="Training step of a SAGE 'mean' teacher (native: one C call per batch; needs --sage_aggregator mean)")
    # not reference flags: the GCNII teacher's teleport and identity-mapping strengths (conf keys `gcnii_alpha`, `gcnii_lamda`, read by
    # Model; docs/GCNII_SEMANTICS.md).  Unset = the conf's value or the paper's defaults 0.1 / 0.5
    p.add_argument("--gcnii_alpha", type=float, default=None, help="alpha of the GCNII teacher's initial residual (default 0.1)")
    p.add_argument("--gcnii_lamda", type=float, default=None, help="lamda of the GCNII teacher's beta_l = log(lamda / l + 1) (default 0.5)")
    # not a reference flag: the DAGNN teacher's number of propagation steps (conf key `dagnn_k`, read by Model; docs/DAGNN_SEMANTICS.md).
    # Unset = the conf's value or the paper's 10
    p.add_argument("--dagnn_k", type=int, default=None, help="Propagation steps K of the DAGNN teacher (default 10)")
    # not a reference flag: the PNA teacher's degree-scaler constant (conf key `pna_delta`, read by Model; docs/PNA_SEMANTICS.md).  Unset =
    # the conf's value, else the mean of log(deg + 1) over the training graph (run_teacher computes and logs it)
    p.add_argument("--pna_delta", type=float, default=None,
                   help="delta of the PNA teacher's degree scalers (default: mean of log(in-degree + 1) over the training graph)")
    # not reference flags: mini-batch training of the full-graph teachers (kinds.FULL_GRAPH_KINDS) on random-walk induced subgraphs (conf keys
    # `subgraph_walk_length`, `subgraph_self_loop`, read by run_transductive / run_inductive; docs/SUBGRAPH_SEMANTICS.md).  --batch_size is then the number of walk roots per batch; 0 = the full-graph step per epoch
    p.add_argument("--subgraph_walk_length", type=int, default=0,
                   help="Train a full-graph teacher on subgraphs induced by random walks of this many steps from --batch_size roots (0: off)")
    p.add_argument("--subgraph_self_loop", type=str, default="keep", choices=["keep", "add"],
                   help="Self entries of those subgraphs (add: one per row, so no row is empty; needs --subgraph_walk_length)")
    args = p.parse_args(argv)
    if not 0 <= args.subgraph_walk_length <= 64:
        p.error(f"--subgraph_walk_length must be in [0, 64] (got {args.subgraph_walk_length})")
    if args.subgraph_walk_length > 0 and teacher_kind(args.teacher) in ("sage", "mlp"):
        p.error(f"--subgraph_walk_length applies to the full-graph teachers ({teacher_names(',')}) only: SAGE trains on "
                f"sampled blocks and MLP on feature batches (got --teacher {args.teacher})")
    if args.subgraph_self_loop != "keep" and args.subgraph_walk_length == 0:
        p.error(f"--subgraph_self_loop {args.subgraph_self_loop} needs --subgraph_walk_length > 0")
    for flag, kind in (("gcnii_alpha", "gcnii"), ("gcnii_lamda", "gcnii"), ("dagnn_k", "dagnn"), ("pna_delta", "pna")):
        if getattr(args, flag) is not None and teacher_kind(args.teacher) != kind:
            p.error(f"--{flag} applies to the {BY_KIND[kind].key} teacher only (got --teacher {args.teacher})")
    if args.dagnn_k is not None and args.dagnn_k < 0:
        p.error(f"--dagnn_k must be >= 0 (got {args.dagnn_k})")
    if args.pna_delta is not None and not args.pna_delta > 0:
        p.error(f"--pna_delta must be positive (got {args.pna_delta})")
    if args.sage_mean_step != "autograd" and ("SAGE" not in args.teacher or args.sage_aggregator != "mean"):
        p.error(f"--sage_mean_step {args.sage_mean_step} applies to --teacher SAGE --sage_aggregator mean only "
                f"(got --teacher {args.teacher} --sage_aggregator {args.sage_aggregator})")
    if args.inference_fan_out.strip():
        if teacher_kind(args.teacher) != "sage":
            p.error(f"--inference_fan_out applies to the SAGE teacher only (got --teacher {args.teacher})")
        try:
            fan_out = [int(f) for f in args.inference_fan_out.split(",")]
        except ValueError:
            p.error(f"--inference_fan_out must be a comma-separated list of integers (got {args.inference_fan_out!r})")
        if len(fan_out) != args.num_layers:
            p.error(f"--inference_fan_out names {len(fan_out)} layers, --num_layers is {args.num_layers} (got {args.inference_fan_out!r})")
        if not all(1 <= f <= 64 for f in fan_out):
            p.error(f"--inference_fan_out values must be in [1, 64] (got {args.inference_fan_out!r})")
    if args.inference_dtype != "float32" and "SAGE" not in args.teacher:
        p.error(f"--inference_dtype {args.inference_dtype} is implemented for the SAGE teacher only (got --teacher {args.teacher})")
    if args.sage_aggregator != "gcn" and "SAGE" not in args.teacher:
        p.error(f"--sage_aggregator {args.sage_aggregator} applies to the SAGE teacher only (got --teacher {args.teacher})")
    if args.sage_aggregator != "gcn" and args.inference_dtype != "float32":
        p.error(f"--sage_aggregator {args.sage_aggregator} runs its inference in float32 only")
    return args


def get_student_args(argv=None):
    p = _parser(_COMMON + _STUDENT_ONLY, "GLNN student distillation (HIP hot path)")
    # not a reference flag: the storage of the student's evaluation / serving passes (train_and_eval.evaluate_mini_batch(dtype=...)),
    # bfloat16 = weights and hidden activations stored as bf16, bf16 MFMA products, fp32 accumulation and saved log-probs (glnn_amd.serve)
    p.add_argument("--serve_dtype", type=str, default="float32", choices=["float32", "bfloat16"],
                   help="Storage of the MLP student's evaluation passes (bfloat16: norm_type none / batch)")
    p.add_argument("--serve_fused", action="store_true",
                   help="Run the bfloat16 evaluation passes as one launch per row block (needs --serve_dtype bfloat16; same results)")
    # not reference flags: DeepWalk position features concatenated to the student's input (glnn_amd.position; docs/POSITION_SEMANTICS.md).
    # --position_dim 0 (the default) is off: nothing changes.  The YAML section is still the plain student's
    p.add_argument("--position_dim", type=int, default=0,
                   help="Width of the DeepWalk position embedding appended to the student's features (0: off; a multiple of 4, <= 256)")
    p.add_argument("--position_walk_length", type=int, default=20, help="Steps per random walk of the position embedding")
    p.add_argument("--position_context", type=int, default=10, help="Skip-gram window (nodes per window) of the position embedding")
    p.add_argument("--position_negatives", type=int, default=1, help="Uniform negatives per positive pair of the position embedding")
    p.add_argument("--position_epochs", type=int, default=5, help="Passes over the nodes (each a walk root once) of the position embedding")
    p.add_argument("--position_batch_size", type=int, default=4096, help="Walk roots per step of the position embedding")
    p.add_argument("--position_lr", type=float, default=0.01, help="Learning rate of the position embedding's lazy Adam")
    # the rest of the node2vec family, each off at its default (the defaults are DeepWalk with uniform negatives and one table)
    p.add_argument("--position_p", type=float, default=1.0, help="node2vec return parameter p of the position walks, in [0.25, 4] (1: unbiased)")
    p.add_argument("--position_q", type=float, default=1.0, help="node2vec in-out parameter q of the position walks, in [0.25, 4] (1: unbiased)")
    p.add_argument("--position_negative_power", type=float, default=0.0,
                   help="Negatives drawn in proportion to degree ** this (0: uniform; 0.75 is the usual value)")
    p.add_argument("--position_context_table", action="store_true",
                   help="Score the entries of a pair against a separate context table (the embedding table stays the output)")
    args = p.parse_args(argv)
    if args.serve_fused and args.serve_dtype != "bfloat16":
        p.error("--serve_fused is a form of the bfloat16 serving path: it needs --serve_dtype bfloat16")
    if not (0.25 <= args.position_p <= 4.0 and 0.25 <= args.position_q <= 4.0):
        p.error(f"--position_p and --position_q must be in [0.25, 4] (got {args.position_p}, {args.position_q})")
    if not args.position_negative_power >= 0.0:
        p.error(f"--position_negative_power must be >= 0 (got {args.position_negative_power})")
    if args.position_dim < 0 or args.position_dim % 4 or args.position_dim > 256:
        p.error(f"--position_dim must be 0 (off) or a multiple of 4 up to 256 (got {args.position_dim})")
    if args.position_dim > 0:
        if not 1 <= args.position_walk_length <= 64:
            p.error(f"--position_walk_length must be in [1, 64] (got {args.position_walk_length})")
        if not 2 <= args.position_context <= args.position_walk_length + 1:
            p.error(f"--position_context must be in [2, --position_walk_length + 1] (got {args.position_context})")
        if args.position_negatives < 1 or args.position_epochs < 1 or args.position_batch_size < 1:
            p.error("--position_negatives, --position_epochs and --position_batch_size must be >= 1")
    return args


def _device(args):
    """The reference maps --device -1 (its default) to the CPU (train_teacher.py:162-165).  This build computes on
    libglnn_hip.so only, so a CPU selection fails HERE -- before any output directory is created -- instead of mid-run."""
    if args.device < 0 or not torch.cuda.is_available():
        raise SystemExit("glnn_amd runs on the MI355X HIP path only and has no CPU path: pass --device 0 (the reference's "
                         f"default --device -1 selects the CPU; torch.cuda.is_available() = {torch.cuda.is_available()})")
    return torch.device("cuda:" + str(args.device))


def _setting_dir(args, root, leaf):
    if args.exp_setting == "tran":
        return Path.cwd().joinpath(root, "transductive", args.dataset, leaf, f"seed_{args.seed}")
    if args.exp_setting == "ind":
        return Path.cwd().joinpath(root, "inductive", f"split_rate_{args.split_rate}", args.dataset, leaf, f"seed_{args.seed}")
    raise ValueError(f"Unknown experiment setting! {args.exp_setting}")


def pna_delta(g):
    """PNA's delta of a training graph: the mean over its rows of log(in-degree + 1), in fp64 (Corso et al., eq. 5; docs/PNA_SEMANTICS.md)."""
    deg = g.in_degrees().cpu().numpy().astype(np.float64)
    return float(np.mean(np.log(deg + 1.0))) if deg.size else 0.0


def _training_config(path, model_name, dataset):
    """get_training_config.  train.conf.yaml has no section for some families (DAGNN, GraphTransformer, PNA: the rows of kinds.KINDS with
    `stand_ins`).  Such a teacher takes the dataset's own section if a user added one, else the first stand-in section the dataset has
    (DAGNN: APPNP's, the trunk's hyper-parameters; PNA: GCN's, those of a conv stack; GraphTransformer: GATv2's, then GAT's, whose conf
    contract it shares), else the global section alone where the row allows it, else raises, naming the two keys a conf must carry."""
    row = BY_KIND[teacher_kind(model_name)]
    if row.stand_ins:
        with open(path) as fh:
            cfg = yaml.safe_load(fh)
        sections = cfg.get(dataset) or {}
        if model_name not in sections:
            for name in row.stand_ins:
                if sections.get(name):
                    return dict(cfg["global"], **sections[name], model_name=model_name)
            if row.global_alone:
                return dict(cfg["global"], model_name=model_name)
            raise ValueError(f"{model_name}: {path} has no {model_name}, {' or '.join(row.stand_ins)} section for dataset {dataset!r}, so "
                             f"nothing names num_heads and attn_dropout_ratio, the two conf keys a {row.key} teacher is built from; add a "
                             f"{model_name} section that carries both")
    return get_training_config(path, model_name, dataset)


def _load(args, logger, model_name):
    g, labels, idx_train, idx_val, idx_test = load_data(args.dataset, args.data_path, split_idx=args.split_idx, seed=args.seed,
                                                        labelrate_train=args.labelrate_train, labelrate_val=args.labelrate_val)
    logger.info(f"Total {g.number_of_nodes()} nodes.")
    logger.info(f"Total {g.number_of_edges()} edges.")
    feats = g.ndata["feat"]
    args.feat_dim = feats.shape[1]
    args.label_dim = labels.int().max().item() + 1
    if 0 < args.feature_noise <= 1:
        feats = (1 - args.feature_noise) * feats + args.feature_noise * torch.randn_like(feats)
    conf = {}
    if args.model_config_path is not None:
        conf = _training_config(args.model_config_path, model_name, args.dataset.replace("synthetic-", "").split("@")[0])
    conf = dict(args.__dict__, **conf)          # YAML wins over CLI flags, as in the reference
    return g, feats, labels, (idx_train, idx_val, idx_test), conf


def _save(args, output_dir, out, loss_and_score, model, g):
    np.savez(output_dir.joinpath("out"), out.detach().cpu().numpy())
    if args.save_results:
        np.savez(output_dir.joinpath("loss_and_score"), np.array(loss_and_score))
        torch.save(model.state_dict(), output_dir.joinpath("model.pth"))
    if args.exp_setting == "tran" and args.compute_min_cut:
        with open(output_dir.parent.joinpath("min_cut_loss"), "a+") as f:
            f.write(f"{compute_min_cut_loss(g.to(out.device), out) :.4f}\n")


def _prop(feats, g, k, device):
    return feature_prop(feats.to(device), g.to(device), k).cpu() if k > 0 else feats


def _with_position(args, feats, g, idx_obs, device, logger):
    """--position_dim D > 0: feats with a DeepWalk embedding of D columns appended (run_student widens conf["feat_dim"] by D).  idx_obs None
    (transductive): fitted on g.  Inductive: fitted on g.subgraph(idx_obs) only, the rows of the hidden test nodes filled with the mean
    over their observed in-neighbours (position.fill_unseen) -- NOSMOG's recipe.  Returns (feats, table): the fitted embedding as a
    position.PositionTable, what serve_student.py serves from (None when --position_dim is 0)."""
    if args.position_dim <= 0:
        return feats, None
    from .position import DeepWalk, PositionTable, fill_unseen
    gd = g.to(device)
    sub = gd if idx_obs is None else g.subgraph(idx_obs).to(device)
    dw = DeepWalk(sub, args.position_dim, args.position_walk_length, args.position_context, args.position_negatives,
                  lr=args.position_lr, seed=args.seed, p=args.position_p, q=args.position_q, negative_power=args.position_negative_power,
                  context_table=args.position_context_table)
    losses = dw.fit(args.position_epochs, args.position_batch_size)
    logger.info(f"position embedding: {sub.num_nodes()} nodes x {args.position_dim}, loss per epoch " + " ".join(f"{x:.4f}" for x in losses))
    z = dw.embedding
    table = PositionTable.from_deepwalk(dw, idx_obs, g.num_nodes())
    if idx_obs is not None:
        full = torch.zeros((g.num_nodes(), args.position_dim), dtype=torch.float32, device=device)
        full[torch.as_tensor(idx_obs, dtype=torch.int64, device=device)] = z
        z = fill_unseen(gd, full, idx_obs)
    return torch.cat([feats, z.to(feats.device)], dim=1), table


def run_teacher(args):
    set_seed(args.seed)
    device = _device(args)
    if args.feature_noise != 0 and args.seed == 0:
        args.output_path = Path.cwd().joinpath(args.output_path, "noisy_features", f"noise_{args.feature_noise}")
    if args.feature_aug_k > 0 and args.seed == 0:
        args.output_path = Path.cwd().joinpath(args.output_path, "aug_features", f"aug_hop_{args.feature_aug_k}")
        args.teacher = f"GA{args.feature_aug_k}{args.teacher}"
    output_dir = _setting_dir(args, args.output_path, args.teacher)
    args.output_dir = output_dir
    check_writable(output_dir, overwrite=False)
    logger = get_logger(output_dir.joinpath("log"), args.console_log, args.log_level)
    logger.info(f"output_dir: {output_dir}")
    g, feats, labels, (idx_train, idx_val, idx_test), conf = _load(args, logger, args.teacher)
    conf["device"] = device
    if teacher_kind(args.teacher) == "pna" and conf.get("pna_delta") is None:
        # a constant of the model, fixed ONCE from the graph the teacher trains on (inductive: the observed graph) and saved with it
        g_train = g if args.exp_setting == "tran" else g.subgraph(graph_split(idx_train, idx_val, idx_test, args.split_rate, args.seed)[3])
        conf["pna_delta"] = pna_delta(g_train)
        logger.info(f"pna_delta: {conf['pna_delta']!r} (mean of log(in-degree + 1) over the {g_train.num_nodes()} nodes of the training graph)")
    logger.info(f"conf: {conf}")
    model = Model(conf)
    optimizer = optim.Adam(model.parameters(), lr=conf["learning_rate"], weight_decay=conf["weight_decay"])
    criterion = torch.nn.NLLLoss()
    evaluator = get_evaluator(conf["dataset"])
    loss_and_score = []
    if args.exp_setting == "tran":
        feats = _prop(feats, g, args.feature_aug_k, device)
        out, score_val, score_test = run_transductive(conf, model, g, feats, labels, (idx_train, idx_val, idx_test), criterion,
                                                      evaluator, optimizer, logger, loss_and_score)
        score_lst = [score_test]
    else:
        indices = graph_split(idx_train, idx_val, idx_test, args.split_rate, args.seed)
        if args.feature_aug_k > 0:
            idx_obs = indices[3]
            obs_feats = _prop(feats[idx_obs], g.subgraph(idx_obs), args.feature_aug_k, device)
            feats = _prop(feats, g, args.feature_aug_k, device)
            feats[idx_obs] = obs_feats
        out, score_val, score_tt, score_ti = run_inductive(conf, model, g, feats, labels, indices, criterion, evaluator, optimizer,
                                                           logger, loss_and_score)
        score_lst = [score_tt, score_ti]
    logger.info(f"num_layers: {conf['num_layers']}. hidden_dim: {conf['hidden_dim']}. dropout_ratio: {conf['dropout_ratio']}")
    logger.info(f"# params {sum(p.numel() for p in model.parameters())}")
    _save(args, output_dir, out, loss_and_score, model, g)
    return score_lst


def run_student(args):
    set_seed(args.seed)
    device = _device(args)
    if args.feature_noise != 0 and args.seed == 0:
        args.output_path = Path.cwd().joinpath(args.output_path, "noisy_features", f"noise_{args.feature_noise}")
        args.out_t_path = args.output_path      # the teacher is assumed trained on the same noisy features
    if args.feature_aug_k > 0 and args.seed == 0:
        args.output_path = Path.cwd().joinpath(args.output_path, "aug_features", f"aug_hop_{args.feature_aug_k}")
        args.student = f"GA{args.feature_aug_k}{args.student}"
    pe = f"PE{args.position_dim}" if args.position_dim > 0 else ""          # runs with position features get a leaf of their own
    output_dir = _setting_dir(args, args.output_path, f"{args.teacher}_{pe}{args.student}")
    out_t_dir = _setting_dir(args, args.out_t_path, args.teacher)
    args.output_dir = output_dir
    check_writable(output_dir, overwrite=False)
    check_readable(out_t_dir)
    logger = get_logger(output_dir.joinpath("log"), args.console_log, args.log_level)
    logger.info(f"output_dir: {output_dir}")
    logger.info(f"out_t_dir: {out_t_dir}")
    g, feats, labels, (idx_train, idx_val, idx_test), conf = _load(args, logger, args.student)     # student section of the YAML
    conf["device"] = device
    conf["feat_dim"] += args.position_dim        # the first layer also takes the position columns (_with_position appends them below)
    logger.info(f"conf: {conf}")
    model = Model(conf)
    optimizer = optim.Adam(model.parameters(), lr=conf["learning_rate"], weight_decay=conf["weight_decay"])
    criterion_l = torch.nn.NLLLoss()
    criterion_t = torch.nn.KLDivLoss(reduction="batchmean", log_target=True)
    evaluator = get_evaluator(conf["dataset"])
    out_t = load_out_t(out_t_dir)
    for nm, idx in (("train", idx_train), ("val", idx_val), ("test", idx_test)):
        logger.debug(f"teacher score on {nm} data: {evaluator(out_t[idx], labels[idx])}")
    loss_and_score = []
    if args.exp_setting == "tran":
        distill_indices = (idx_train, torch.cat([idx_train, idx_val, idx_test]), idx_val, idx_test)
        feats = _prop(feats, g, args.feature_aug_k, device)
        feats, table = _with_position(args, feats, g, None, device, logger)
        out, score_val, score_test = distill_run_transductive(conf, model, feats, labels, out_t, distill_indices, criterion_l,
                                                              criterion_t, evaluator, optimizer, logger, loss_and_score)
        score_lst = [score_test]
    else:
        obs_idx_train, obs_idx_val, obs_idx_test, idx_obs, idx_test_ind = graph_split(idx_train, idx_val, idx_test, args.split_rate, args.seed)
        distill_indices = (obs_idx_train, torch.cat([obs_idx_train, obs_idx_val, obs_idx_test]), obs_idx_val, obs_idx_test,
                           idx_obs, idx_test_ind)
        if args.feature_aug_k > 0:
            obs_feats = _prop(feats[idx_obs], g.subgraph(idx_obs), args.feature_aug_k, device)
            feats = _prop(feats, g, args.feature_aug_k, device)
            feats[idx_obs] = obs_feats
        feats, table = _with_position(args, feats, g, idx_obs, device, logger)
        out, score_val, score_tt, score_ti = distill_run_inductive(conf, model, feats, labels, out_t, distill_indices, criterion_l,
                                                                   criterion_t, evaluator, optimizer, logger, loss_and_score)
        score_lst = [score_tt, score_ti]
    logger.info(f"num_layers: {conf['num_layers']}. hidden_dim: {conf['hidden_dim']}. dropout_ratio: {conf['dropout_ratio']}")
    logger.info(f"# params {sum(p.numel() for p in model.parameters())}")
    _save(args, output_dir, out, loss_and_score, model, g)
    if table is not None and args.save_results:
        table.save(output_dir.joinpath("position.npz"))          # what serve_student.py serves from, beside model.pth
    return score_lst


SERVE_BATCH_IDS = 4096         # serve_student.py: ids per call of the served chain (see run_serve)


def get_serve_args(argv=None):
    """serve_student.py: the flags that locate a finished train_student.py run (the student's own flags, with the same defaults and the
    same YAML merge), --serve_dtype, --serve_fused and --nodes."""
    p = _parser(_COMMON + _STUDENT_ONLY, "GLNN position-feature student: serve saved artefacts by node id (HIP hot path)")
    p.add_argument("--serve_dtype", type=str, default="float32", choices=["float32", "bfloat16"],
                   help="Storage of the served chain (bfloat16: bf16 weights, activations and assembled rows)")
    p.add_argument("--serve_fused", action="store_true",
                   help="Run the bfloat16 chain as one launch per assembled block (needs --serve_dtype bfloat16; same results)")
    p.add_argument("--position_dim", type=int, default=0, help="--position_dim of the run to serve (it names the run's directory)")
    p.add_argument("--nodes", type=str, default=None, help="An .npy of int64 node ids to serve (default: every node)")
    args = p.parse_args(argv)
    if args.serve_fused and args.serve_dtype != "bfloat16":
        p.error("--serve_fused is a form of the bfloat16 serving path: it needs --serve_dtype bfloat16")
    if args.feature_aug_k > 0:
        p.error("serve_student.py does not serve --feature_aug_k runs: the augmented features are propagated over the graph at training "
                "time and are not a saved artefact")
    if args.feature_noise != 0:
        p.error("serve_student.py does not serve --feature_noise runs: the noise drawn at training time is not a saved artefact")
    if args.position_dim < 0 or args.position_dim % 4 or args.position_dim > 256:
        p.error(f"--position_dim must be 0 or a multiple of 4 up to 256 (got {args.position_dim})")
    return args


def run_serve(args):
    """Log-probabilities of --nodes from the artefacts of a train_student.py --position_dim D --save_results run: the dataset's features,
    model.pth and position.npz, through serve.compile_position_student; writes served_out.npz (arr_0: [len(nodes), C] float32) into the
    run's directory."""
    pe = f"PE{args.position_dim}" if args.position_dim > 0 else ""
    output_dir = _setting_dir(args, args.output_path, f"{args.teacher}_{pe}{args.student}")
    for name, why in (("position.npz", "only runs with --position_dim D > 0 and --save_results write it"),
                      ("model.pth", "only runs with --save_results write it")):
        if not output_dir.joinpath(name).exists():
            raise SystemExit(f"serve_student.py: {output_dir} has no {name} ({why}); nothing to serve")
    device = _device(args)
    import logging
    from .position import PositionTable
    from .serve import compile_position_student
    from .train_and_eval import INFERENCE_DTYPES
    g, feats, _, _, conf = _load(args, logging.getLogger("glnn_amd.serve_student"), args.student)
    table = PositionTable.load(output_dir.joinpath("position.npz"), device)
    if table.dim != args.position_dim:
        raise SystemExit(f"serve_student.py: position.npz holds rows of {table.dim} columns, --position_dim says {args.position_dim}")
    conf["device"] = device
    conf["feat_dim"] += table.dim
    model = Model(conf)
    model.load_state_dict(torch.load(output_dir.joinpath("model.pth"), map_location=device))
    model.eval()
    n = g.num_nodes()
    needs_graph = table.has_unseen or n > table.num_nodes
    served = compile_position_student(model, feats.to(device), table, g.to(device) if needs_graph else None,
                                      dtype=INFERENCE_DTYPES[args.serve_dtype], fused=args.serve_fused)
    nodes = torch.arange(n, dtype=torch.int64) if args.nodes is None else torch.from_numpy(np.load(args.nodes).astype(np.int64).reshape(-1))
    if nodes.numel() and (int(nodes.min()) < 0 or int(nodes.max()) >= n):
        raise SystemExit(f"serve_student.py: --nodes must hold node ids in [0, {n}) (got {int(nodes.min())} .. {int(nodes.max())})")
    # Fixed batches: the fp32 chain picks its GEMM form (latency kernels, split-K) by the row count of the call, so the bits of a row depend
    # on how many rows it was served with.  Every call here has SERVE_BATCH_IDS rows, the last batch padded by repeating its last id: what
    # a node is served does not depend on the request it came in.
    nodes = nodes.to(device)
    out = torch.empty((nodes.numel(), conf["label_dim"]), dtype=torch.float32, device=device)
    batch = torch.empty((SERVE_BATCH_IDS, conf["label_dim"]), dtype=torch.float32, device=device)
    for s0 in range(0, nodes.numel(), SERVE_BATCH_IDS):
        sub = nodes[s0:s0 + SERVE_BATCH_IDS]
        k = sub.numel()
        if k < SERVE_BATCH_IDS:
            sub = torch.cat([sub, sub[-1:].expand(SERVE_BATCH_IDS - k)])
        served.log_probs(sub, out=batch, check_ids=False)
        out[s0:s0 + k] = batch[:k]
    np.savez(output_dir.joinpath("served_out"), out.cpu().numpy())
    return out


def serve_main(argv=None):
    out = run_serve(get_serve_args(argv))
    print(f"served {out.shape[0]} nodes")


def _main(args, run):
    if args.num_exp == 1:
        score = run(args)
        score_str = "".join([f"{s : .4f}\t" for s in score])
    else:
        scores = []
        for seed in range(args.num_exp):
            args.seed = seed
            scores.append(run(args))
        scores = np.array(scores)
        score_str = "".join([f"{s : .4f}\t" for s in scores.mean(axis=0)] + [f"{s : .4f}\t" for s in scores.std(axis=0)])
    with open(args.output_dir.parent.joinpath("exp_results"), "a+") as f:
        f.write(f"{score_str}\n")
    print(score_str)      # for collecting aggregated results


def teacher_main(argv=None):
    _main(get_teacher_args(argv), run_teacher)


def student_main(argv=None):
    _main(get_student_args(argv), run_student)
