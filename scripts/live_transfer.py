#!/usr/bin/env python
"""Timbre transfer of one recording on MI355X as a live input would be served: the whole chain chunk by chunk, every stage a
stream that keeps its state on the GPU.

    wav --chunk samples at a time -> [StreamResampler to the model's rate, where the file's differs] -> StreamControl (pYIN F0 +
    loudness with a fixed lag, normalised with the checkpoint's statistics) -> model.stream(1).push whenever frames come out
    -> [StreamResampler to --output-rate] -> wav

    python scripts/live_transfer.py in.wav out.wav [--model-checkpoint ckpt] [--normalisation-dir dir] [--use-fastnewt]
                                    [--chunk N] [--lag L] [--loudness-reference running|FLOAT_DBFS] [--loudness-release DB_PER_S]
                                    [--output-rate R] [--seed S]

--loudness-reference running measures the loudness against the loudest power heard so far (a quiet start is
rendered too loud until the peak has been heard); a number fixes the reference at the level of a sine of that many dBFS
(0 = full scale), a calibration.  --loudness-release DB_PER_S lets the running reference fall by that many dB per second
(DESIGN.md 3.26), so that the level recovers after a click; 0, the default, keeps it where the loudest sound put it.  The script prints the chain's latency: the samples by which the output runs behind the input.
The output has the input's length (at the model's rate, converted to --output-rate where given).  --seed fixes the model's two
random draws, so that two runs write the same file.
"""
import importlib
import os
import sys

import click
import numpy as np
import torch
from scipy.io import wavfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from timbre_transfer import normalisation  # noqa: E402


def read_left(path, pre):
    """float32, mono (left channel) at the file's own rate"""
    sr, x = wavfile.read(path)
    if x.dtype == np.uint8:
        x = (x.astype(np.float32) - 128.0) / 128.0
    elif x.dtype == np.float64:
        x = x.astype(np.float32)
    return int(sr), np.ascontiguousarray(pre.make_monophonic(pre.convert_to_float32_audio(x)), dtype=np.float32)


def sine_power(dbfs, n_fft=1024):
    """power of the peak bin of a sine of `dbfs` under the periodic hann window: (A n_fft / 4)^2"""
    return (10.0 ** (dbfs / 20.0) * n_fft / 4.0) ** 2


@click.command()
@click.argument("input_wav", type=click.Path(exists=True))
@click.argument("output_wav", type=click.Path())
@click.option("--model-gin", default=None)
@click.option("--model-checkpoint", default=os.path.join(ROOT, "tests", "golden", "weights_vn.npz"), show_default=True)
@click.option("--normalisation-dir", default=None, help="directory of data_mean.npy / data_std.npy (default: the checkpoint's)")
@click.option("--use-fastnewt", is_flag=True)
@click.option("--octave-shift", default=0, type=int, help="transpose the extracted F0 by whole octaves")
@click.option("--chunk", default=256, type=click.IntRange(1), show_default=True, help="samples of the input file per push")
@click.option("--lag", default=8, type=click.IntRange(0, 255), show_default=True, help="frames the analysis looks ahead")
@click.option("--loudness-reference", default="running", show_default=True, help="running, or the reference level in dBFS of a sine")
@click.option("--loudness-release", default=0.0, type=click.FloatRange(0.0), show_default=True,
              help="dB per second by which the running reference falls (0: it never falls)")
@click.option("--output-rate", default=None, type=int, help="convert the model's output to this sample rate")
@click.option("--seed", default=None, type=int, help="seed torch's generators, so that two runs draw the same start phases and noise")
def main(input_wav, output_wav, model_gin, model_checkpoint, normalisation_dir, use_fastnewt, octave_shift, chunk, lag,
         loudness_reference, loudness_release, output_rate, seed):
    nws = importlib.import_module("neural-waveshaping-synthesis_amd")
    ck = importlib.import_module("neural-waveshaping-synthesis_amd.checkpoint")
    pre = importlib.import_module("neural-waveshaping-synthesis_amd.data.utils.preprocess_audio")
    streaming = importlib.import_module("neural-waveshaping-synthesis_amd.streaming")
    if loudness_reference != "running":
        try:
            loudness_reference = sine_power(float(loudness_reference))
        except ValueError:
            raise click.BadParameter(f"--loudness-reference {loudness_reference}: expected 'running' or a level in dBFS")
        if loudness_release > 0.0:
            raise click.BadParameter("--loudness-release belongs to --loudness-reference running: a fixed reference does not move")
    if model_gin:
        nws.gin.parse_config_file(model_gin)
    else:
        nws.ensure_default_config()
    model = nws.NeuralWaveshaping.load_from_checkpoint(model_checkpoint).eval()
    if use_fastnewt:
        model.newt = nws.FastNEWT(model.newt)
    model = model.cuda()
    sr, hop = int(model.sample_rate), int(model.control_hop)
    mean, std = normalisation(ck, model_checkpoint, normalisation_dir)
    sr_in, audio = read_left(input_wav, pre)
    if seed is not None:
        torch.manual_seed(seed)

    to_model = streaming.StreamResampler(sr_in, sr, 1) if sr_in != sr else None
    control = streaming.StreamControl(model, 1, lag=lag, reference=loudness_reference, mean=mean, std=std, octave_shift=octave_shift,
                                      release_db_per_s=loudness_release)
    synth = model.stream(1)
    to_output = streaming.StreamResampler(sr, output_rate, 1) if output_rate is not None and output_rate != sr else None
    # the output runs behind the input by: the converter's look-ahead, half an analysis frame + the lag, the 64 samples the
    # model's linear upsampling looks ahead, the second converter's look-ahead - each in its own rate
    parts = [(to_model.latency_samples, sr_in)] if to_model else []
    parts += [(control.latency_samples, sr), (hop // 2, sr)]
    parts += [(to_output.latency_samples, sr)] if to_output else []
    latency_ms = sum(1e3 * n / rate for n, rate in parts)

    x = torch.from_numpy(audio).cuda().unsqueeze(0)
    pieces, frames, n_model, rendered = [], 0, 0, 0
    for at in range(0, audio.size, chunk):
        last = at + chunk >= audio.size
        piece = x[:, at:at + chunk]
        if to_model:
            piece = to_model.push(piece, final=last)
        n_model += piece.shape[1]
        if piece.shape[1] == 0 and not last:
            continue
        f0, c = control.push(piece, final=last)
        if f0.shape[2] == 0:
            continue
        frames += f0.shape[2]
        with torch.no_grad():
            y = synth.push(f0, c, final=last)
        if last:
            y = y[:, :max(0, n_model - rendered)]                  # the model renders whole frames: cut to the input's length
        rendered += y.shape[1]
        pieces.append(to_output.push(y, final=last) if to_output else y)
    y = torch.cat(pieces, dim=1)[0].cpu().numpy().astype(np.float32)
    wavfile.write(output_wav, output_rate if to_output else sr, y)
    print(f"{input_wav}: {audio.size} samples at {sr_in} Hz in chunks of {chunk}, {frames} frames, lag {lag} -> {output_wav}: "
          f"{y.size} samples at {output_rate if to_output else sr} Hz; latency of the chain "
          + " + ".join(f"{n} samples at {rate} Hz" for n, rate in parts) + f" = {latency_ms:.1f} ms")


if __name__ == "__main__":
    main()
