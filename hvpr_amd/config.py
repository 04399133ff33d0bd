"""yaml -> attribute dict, with the reference's `_BASE_CONFIG_` include and recursive merge semantics
(pcdet/config.py:51-85).  easydict is not a dependency: AttrDict is the small subset the models use."""
import os

import yaml


class AttrDict(dict):
    def __init__(self, d=None, **kw):
        super().__init__()
        for k, v in dict(d or {}, **kw).items():
            self[k] = v

    def __setitem__(self, k, v):
        super().__setitem__(k, _wrap(v))

    def __setattr__(self, k, v):
        self[k] = v

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None


def _wrap(v):
    if isinstance(v, dict) and not isinstance(v, AttrDict):
        return AttrDict(v)
    if isinstance(v, (list, tuple)):
        return [_wrap(x) for x in v]
    return v


def _get(cfg, key, default=None):
    """cfg[key], or `default` where the block has no such key."""
    return cfg[key] if key in cfg else default


def _has_include(d):
    return isinstance(d, dict) and ("_BASE_CONFIG_" in d or any(_has_include(v) for v in d.values()))


def _merge(config, new, base_dir):
    if "_BASE_CONFIG_" in new:
        path = new["_BASE_CONFIG_"]
        if not os.path.isabs(path):
            for root in (os.getcwd(), base_dir, os.path.dirname(base_dir)):
                if os.path.exists(os.path.join(root, path)):
                    path = os.path.join(root, path)
                    break
        with open(path) as f:
            base = yaml.safe_load(f)
        if _has_include(base):
            _merge(config, base, base_dir)        # a base that includes files itself, at any depth (a model yaml as the base of another one)
        else:
            config.update(AttrDict(base))
    for k, v in new.items():
        if not isinstance(v, dict):
            config[k] = v
            continue
        if k not in config:
            config[k] = AttrDict()
        _merge(config[k], v, base_dir)
    return config


def cfg_from_yaml_file(cfg_file, config=None):
    config = AttrDict() if config is None else config
    with open(cfg_file) as f:
        new = yaml.safe_load(f)
    return _merge(config, new, os.path.dirname(os.path.dirname(os.path.abspath(cfg_file))))


def _literal(text):
    import ast
    try:
        return ast.literal_eval(text)
    except (ValueError, SyntaxError):
        return text


def cfg_from_list(cfg_list, config):
    """`--set KEY VALUE ...` (pcdet/config.py:24-48): KEY is a dotted path that must exist; VALUE is read as a Python literal (a bare
    word stays a string) and must have the type of the value it replaces.  A value for a list may be written `a,b,c`; its items
    take the type of the list's first item.  An int is taken for a float."""
    if len(cfg_list) % 2 != 0:
        raise ValueError("--set takes KEY VALUE pairs")
    for key, text in zip(cfg_list[0::2], cfg_list[1::2]):
        d = config
        parts = key.split(".")
        for p in parts[:-1]:
            if not isinstance(d, dict) or p not in d:
                raise KeyError(f"--set {key}: no such key")
            d = d[p]
        last = parts[-1]
        if not isinstance(d, dict) or last not in d:
            raise KeyError(f"--set {key}: no such key")
        old = d[last]
        new = _literal(text) if isinstance(text, str) else text
        if isinstance(old, dict):
            raise TypeError(f"--set {key}: a block cannot be replaced, set its keys")
        if isinstance(old, list) and isinstance(new, str):
            items = new.split(",")
            new = [type(old[0])(_literal(x)) for x in items] if old else [_literal(x) for x in items]
        if isinstance(new, tuple):
            new = list(new)
        if isinstance(old, float) and isinstance(new, int) and not isinstance(new, bool):
            new = float(new)
        if old is not None and type(new) is not type(old):
            raise TypeError(f"--set {key}: {type(new).__name__} given for a {type(old).__name__}")
        d[last] = new
    return config


CFG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cfgs")


def hvpr_car_cfg():
    return cfg_from_yaml_file(os.path.join(CFG_DIR, "kitti_models", "hvpr_car.yaml"))


def hvpr_car_atss_cfg():
    """hvpr_car.yaml with TARGET_ASSIGNER_CONFIG.NAME: ATSS, TOPK 9."""
    return cfg_from_yaml_file(os.path.join(CFG_DIR, "kitti_models", "hvpr_car_atss.yaml"))


def pointpillar_cfg():
    """Plain PointPillars, KITTI 3-class, 432 x 496 pillars (eval only)."""
    return cfg_from_yaml_file(os.path.join(CFG_DIR, "kitti_models", "pointpillar.yaml"))


def hvpr_3class_cfg():
    """BASELINE.json configs[3]: Car / Pedestrian / Cyclist, 6 anchors per location."""
    return cfg_from_yaml_file(os.path.join(CFG_DIR, "kitti_models", "hvpr_3class.yaml"))
