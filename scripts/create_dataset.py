#!/usr/bin/env python
"""A folder of wav files -> a dataset of audio segments and normalised control features (F0, loudness, confidence, MFCC) in
the layout scripts/resynthesise_dataset.py reads.  Resampling and the three extractors run on the MI355X.

    python scripts/create_dataset.py --gin-file neural-waveshaping-synthesis_amd/gin/data/urmp_4second_pyin.gin \
        --data-directory recordings/ --output-directory data/
"""
import importlib
import os
import random
import sys

import click
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wav_files(directory):
    """the wav files of a folder, by name"""
    return [os.path.join(directory, name) for name in sorted(os.listdir(directory)) if name.lower().endswith(".wav")]


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


@click.command()
@click.option("--gin-file", required=True, type=click.Path(exists=True, dir_okay=False), help="data configuration, e.g. gin/data/urmp_4second_pyin.gin")
@click.option("--data-directory", required=True, type=click.Path(exists=True, file_okay=False), help="folder of wav files")
@click.option("--output-directory", required=True, help="root of the dataset to write")
@click.option("--seed", default=0, help="governs the assignment of segments to splits")
@click.option("--device", default="cuda", help="value of the %device macro a gin file may refer to")
def main(gin_file, data_directory, output_directory, seed, device):
    nws = importlib.import_module("neural-waveshaping-synthesis_amd")
    cd = importlib.import_module("neural-waveshaping-synthesis_amd.data.utils.create_dataset")
    nws.gin.constant("device", device)
    nws.gin.parse_config_file(gin_file)
    seed_all(seed)
    cd.create_dataset(wav_files(data_directory), output_directory)


if __name__ == "__main__":
    main()
