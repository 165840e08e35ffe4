"""Generic PSNR training driver (the counterpart of the reference's main_train_psnr.py, restated on this package's
surface): every dataset / model / network that define_Dataset / define_Model / define_G accept -- SwinIR, RRDBNet,
USRNet, DRUNet, FFDNet, DnCNN ... -- trained by one loop and validated on the test set.

    python -m kair_amd.main_train_psnr -opt FILE

Same skeleton as main_train_dncnn: parse -> find_last_checkpoint -> seeds -> define_Dataset per phase + DataLoader ->
define_Model -> init_train -> per step: update_learning_rate (before the step), feed_data, optimize_parameters, log /
save / test.  No BatchNorm merging.  gpu_ids null runs it on the host, gpu_ids [0] on the MI355X.

Test phase (every train.checkpoint_test steps), border = opt["scale"] as the reference driver: per test image
feed_data, test(), ModelPlain.test_metrics.  On the GPU the metrics are kair_image_metrics (csrc/metrics.hip) and stay
device tensors; they are concatenated and read ONCE after the loop, so nothing but the forwards and the metric kernels
runs between two test images.  Logged: the average PSNR (two decimals) and, when computed, the average SSIM (four).

Additions (absent from reference option files; the defaults are the reference driver's behaviour):
train.test_y_channel (false): the metrics on the Y channel of RGB images; train.test_ssim (false): SSIM beside PSNR;
train.max_iter ends the run; train.manual_seed.
"""
import argparse
import logging
import math
import os
import random
import sys

import numpy as np
import torch
from torch.utils.data import DataLoader

from .data.select_dataset import define_Dataset
from .models.select_model import define_Model
from .utils import utils_option as option


def validate(model, test_loader, border, y_channel, ssim):
    """(average PSNR, average SSIM or None) over the test set: per-image test_metrics tensors on the model's device,
    one host read at the end."""
    results = []
    for test_data in test_loader:
        model.feed_data(test_data)
        model.test()
        results.append(model.test_metrics(border=border, y_channel=y_channel, ssim=ssim))
    vals = torch.cat(results).tolist()   # the one device -> host read; averaged in image order like the reference loop
    n = len(vals)
    return sum(v[0] for v in vals) / n, (sum(v[1] for v in vals) / n if ssim else None)


def main(json_path, overrides=None, log_stream=None):
    opt = option.parse(json_path, is_train=True)
    if overrides:
        overrides(opt)
    for key, path in opt["path"].items():
        if "pretrained" not in key and isinstance(path, str):
            os.makedirs(path, exist_ok=True)
    init_iter, init_path_G = option.find_last_checkpoint(opt["path"]["models"], net_type="G")
    opt["path"]["pretrained_netG"] = init_path_G
    current_step = init_iter
    border = opt["scale"]
    option.save(opt)
    opt = option.dict_to_nonedict(opt)

    logger = logging.getLogger("kair_amd.train_psnr")
    logger.setLevel(logging.INFO)
    if log_stream is not None or not logger.handlers:   # (a second run in one process logs to its own stream)
        for h in list(logger.handlers):
            logger.removeHandler(h)
        logger.addHandler(logging.StreamHandler(log_stream or sys.stdout))

    seed = opt["train"]["manual_seed"]
    if seed is None:
        seed = random.randint(1, 10000)
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)

    train_loader = test_loader = None
    for phase, ds in opt["datasets"].items():
        dset = define_Dataset(ds)
        if phase == "train":
            logger.info("Number of train images: {:,d}, iters: {:,d}".format(
                len(dset), int(math.ceil(len(dset) / ds["dataloader_batch_size"]))))
            train_loader = DataLoader(dset, batch_size=ds["dataloader_batch_size"], shuffle=ds["dataloader_shuffle"],
                                      num_workers=ds["dataloader_num_workers"] or 0, drop_last=True,
                                      pin_memory=torch.cuda.is_available())
        elif phase == "test":
            test_loader = DataLoader(dset, batch_size=1, shuffle=False, num_workers=0, drop_last=False)

    model = define_Model(opt)
    model.init_train()

    max_iter = opt["train"]["max_iter"]
    y_channel, ssim = bool(opt["train"]["test_y_channel"]), bool(opt["train"]["test_ssim"])
    history = {"loss": [], "psnr": [], "ssim": []}
    done = False
    for epoch in range(1000000):
        for train_data in train_loader:
            current_step += 1
            model.update_learning_rate(current_step)
            model.feed_data(train_data)
            model.optimize_parameters(current_step)
            history["loss"].append(model.current_log()["G_loss"])
            if current_step % opt["train"]["checkpoint_print"] == 0:
                msg = "<epoch:{:3d}, iter:{:8,d}, lr:{:.3e}> ".format(epoch, current_step, model.current_learning_rate())
                msg += " ".join("{:s}: {:.3e}".format(k, v) for k, v in model.current_log().items())
                logger.info(msg)
            if current_step % opt["train"]["checkpoint_save"] == 0:
                model.save(current_step)
            if test_loader is not None and current_step % opt["train"]["checkpoint_test"] == 0:
                avg_psnr, avg_ssim = validate(model, test_loader, border, y_channel, ssim)
                history["psnr"].append((current_step, avg_psnr))
                msg = "<epoch:{:3d}, iter:{:8,d}, Average PSNR : {:<.2f}dB".format(epoch, current_step, avg_psnr)
                if ssim:
                    history["ssim"].append((current_step, avg_ssim))
                    msg += ", Average SSIM : {:<.4f}".format(avg_ssim)
                logger.info(msg)
            if max_iter is not None and current_step >= max_iter:
                done = True
                break
        if done:
            break
    model.save("latest")
    return model, history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("-opt", type=str, required=True)
    main(ap.parse_args().opt)
