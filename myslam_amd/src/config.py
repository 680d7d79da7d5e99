"""Mirror of reference src/config.py:26-92 + src/networks/config.py:25-32: the YAML config reader with `inherit_from`
and the model factory."""
import os


def update_recursive(dict1, dict2):
    """dict2's entries written over dict1's, dictionaries merged key by key (src/config.py:61-75)."""
    for k, v in dict2.items():
        if k not in dict1:
            dict1[k] = dict()
        if isinstance(v, dict):
            update_recursive(dict1[k], v)
        else:
            dict1[k] = v


def _resolve(inherit, path):
    """`inherit_from` as written (relative to the working directory, which is where the reference is run from); when no
    such file exists, against each ancestor directory of the config that names it, nearest first - the reference's
    configs say `configs/Replica/replica.yaml`, so a config tree resolves from any working directory."""
    if os.path.exists(inherit) or os.path.isabs(inherit):
        return inherit
    d = os.path.dirname(os.path.abspath(path))
    while True:
        cand = os.path.join(d, inherit)
        if os.path.exists(cand):
            return cand
        up = os.path.dirname(d)
        if up == d:
            return inherit                   # (open() then names the path as written in its error)
        d = up


def load_config(path, default_path=None):
    """src/config.py:26-58: the file at `path` over the config its `inherit_from` names (recursively), else over
    `default_path` when given."""
    import yaml
    with open(path, 'r') as f:
        cfg_special = yaml.full_load(f)
    inherit_from = cfg_special.get('inherit_from')
    if inherit_from is not None:
        cfg = load_config(_resolve(inherit_from, path), default_path)
    elif default_path is not None:
        with open(default_path, 'r') as f:
            cfg = yaml.full_load(f)
    else:
        cfg = dict()
    update_recursive(cfg, cfg_special)
    return cfg


def get_model(cfg):
    from .networks.decoders import Decoders
    return Decoders(c_dim=cfg['model']['c_dim'], truncation=cfg['model']['truncation'],
                    learnable_beta=cfg['rendering']['learnable_beta'])
