#!/usr/bin/env python
"""Timbre transfer of one recording on MI355X: wav -> pYIN F0 + perceptual loudness (the two analysis kernels) -> control
features normalised with the checkpoint's statistics -> the model -> wav.  The chain of the reference's
data/utils/preprocess_audio.py followed by its inference notebook, on the GPU end to end.

    python scripts/timbre_transfer.py in.wav out.wav --model-checkpoint ckpt [--normalisation-dir dir] [--use-fastnewt]
                                      [--resample] [--output-rate R] [--stream-f0 LAG] [--stream-loudness LAG
                                      [--loudness-reference running|clip] [--loudness-release DB_PER_S]] [--chunk N] [--seed S]

Without --resample the wav must already be at the model's sample rate and mono.  With it the file may be at any rate and
stereo: the left channel is kept and converted to the model's rate on the GPU (csrc/resample.hip), and the output has the
converted length.  --output-rate converts the model's output to another rate with the same kernel.
--stream-f0 LAG takes F0 from the fixed-lag stream (streaming.StreamF0) fed --chunk samples at a time, as a live
input would deliver them, instead of from the offline extractor: everything else runs as without it, so the output lets one
hear what a lag of LAG frames costs (a lag of the whole clip's frame count, at most 255, gives the same file when both runs
fix the model's two random draws - the oscillators' start phases and the noise - with the same --seed).
--stream-loudness LAG takes the loudness from the loudness stream (streaming.StreamLoudness) the same way.
--loudness-reference running measures every frame against the loudest power heard up to LAG frames after it, as a live input
must (a lag of the whole clip's frame count gives the plain run's file); clip fixes the reference at the clip's own peak power
(loudness_extraction.peak_power), which gives the plain run's file at any lag.  --loudness-release DB_PER_S lets the running
reference fall by that many dB per second; 0, the default, is the stream without a release.
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


def read_mono(path, sample_rate):
    sr, x = wavfile.read(path)
    if sr != sample_rate:
        raise click.BadParameter(f"{path} is at {sr} Hz, the model at {sample_rate} Hz: pass --resample, or resample it first")
    if x.ndim != 1:
        raise click.BadParameter(f"{path} has {x.shape[1]} channels: expected a mono file")
    if x.dtype == np.uint8:
        x = (x.astype(np.float64) - 128.0) / 128.0
    elif np.issubdtype(x.dtype, np.integer):
        x = x.astype(np.float64) / (float(np.iinfo(x.dtype).max) + 1.0)
    return np.ascontiguousarray(x, dtype=np.float32)


def read_any(path, sample_rate, pre):
    """--resample: the reference's front end (preprocess_audio.py:109-117): float32, mono (left channel), the model's rate"""
    sr, x = wavfile.read(path)
    if x.dtype == np.uint8:
        x = (x.astype(np.float32) - 128.0) / 128.0
    elif x.dtype == np.float64:
        x = x.astype(np.float32)
    x = np.ascontiguousarray(pre.make_monophonic(pre.convert_to_float32_audio(x)))
    return x if sr == sample_rate else pre.resample_audio(x, sr, sample_rate)


def normalisation(ck, checkpoint, directory):
    directory = directory or os.path.dirname(os.path.abspath(checkpoint))
    if os.path.exists(os.path.join(directory, "data_mean.npy")):
        return ck.load_normalisation(directory)
    if str(checkpoint).endswith(".npz"):
        z = np.load(checkpoint)
        if "__data_mean__" in z.files:
            return z["__data_mean__"].astype(np.float64).reshape(-1), z["__data_std__"].astype(np.float64).reshape(-1)
    raise click.BadParameter(f"no data_mean.npy / data_std.npy in {directory}: pass --normalisation-dir")


def stream_f0_frames(audio, sr, hop, lag, chunk):
    """F0 and voiced probability of every frame through streaming.StreamF0, `chunk` samples a push; numpy like the offline call"""
    streaming = importlib.import_module("neural-waveshaping-synthesis_amd.streaming")
    s = streaming.StreamF0(1, sample_rate=sr, frame_length=1024, hop_length=hop, lag=lag)
    x = torch.from_numpy(audio).cuda().unsqueeze(0)
    outs = [s.push(x[:, at:at + chunk], final=at + chunk >= audio.size) for at in range(0, audio.size, chunk)]
    f0 = torch.cat([o[0] for o in outs], dim=1)[0].cpu().numpy().astype(np.float64)
    return f0, torch.cat([o[1] for o in outs], dim=1)[0].cpu().numpy()


def stream_loudness_frames(audio, hop, lag, chunk, reference, release_db_per_s=0.0, sample_rate=16000):
    """loudness of every frame through streaming.StreamLoudness, `chunk` samples a push; numpy like the offline call"""
    streaming = importlib.import_module("neural-waveshaping-synthesis_amd.streaming")
    ldx = importlib.import_module("neural-waveshaping-synthesis_amd.data.utils.loudness_extraction")
    x = torch.from_numpy(audio).cuda().unsqueeze(0)
    s = streaming.StreamLoudness(1, n_fft=1024, hop_length=hop, lag=lag,
                                 reference="running" if reference == "running" else ldx.peak_power(x, 1024, hop),
                                 release_db_per_s=release_db_per_s, sample_rate=sample_rate)
    outs = [s.push(x[:, at:at + chunk], final=at + chunk >= audio.size) for at in range(0, audio.size, chunk)]
    return torch.cat([o[0] for o in outs], dim=1)[0].cpu().numpy()


@click.command()
@click.argument("input_wav", type=click.Path(exists=True))
@click.argument("output_wav", type=click.Path())
@click.option("--model-gin", default=None)
@click.option("--model-checkpoint", default=os.path.join(ROOT, "tests", "golden", "weights_vn.npz"), show_default=True)
@click.option("--normalisation-dir", default=None, help="directory of data_mean.npy / data_std.npy (default: the checkpoint's)")
@click.option("--use-fastnewt", is_flag=True)
@click.option("--octave-shift", default=0, type=int, help="transpose the extracted F0 by whole octaves")
@click.option("--resample", is_flag=True, help="accept any sample rate and stereo: keep the left channel, convert to the model's rate")
@click.option("--output-rate", default=None, type=int, help="convert the model's output to this sample rate")
@click.option("--stream-f0", default=None, type=click.IntRange(0, 255), help="F0 from the fixed-lag stream with this lag in frames")
@click.option("--stream-loudness", default=None, type=click.IntRange(0, 255), help="loudness from the loudness stream with this lag in frames")
@click.option("--loudness-reference", default="running", type=click.Choice(["running", "clip"]), show_default=True,
              help="reference level of --stream-loudness: the running maximum, or fixed at the clip's peak power")
@click.option("--loudness-release", default=0.0, type=click.FloatRange(0.0), show_default=True,
              help="dB per second by which the running reference of --stream-loudness falls (0: it never falls)")
@click.option("--chunk", default=128, type=click.IntRange(1), show_default=True, help="samples per push of the streams")
@click.option("--seed", default=None, type=int, help="seed torch's generators, so that two runs draw the same start phases and noise")
def main(input_wav, output_wav, model_gin, model_checkpoint, normalisation_dir, use_fastnewt, octave_shift, resample, output_rate,
         stream_f0, stream_loudness, loudness_reference, loudness_release, chunk, seed):
    if loudness_release > 0.0 and (stream_loudness is None or loudness_reference != "running"):
        raise click.BadParameter("--loudness-release belongs to --stream-loudness with --loudness-reference running")
    nws = importlib.import_module("neural-waveshaping-synthesis_amd")
    ck = importlib.import_module("neural-waveshaping-synthesis_amd.checkpoint")
    f0x = importlib.import_module("neural-waveshaping-synthesis_amd.data.utils.f0_extraction")
    ldx = importlib.import_module("neural-waveshaping-synthesis_amd.data.utils.loudness_extraction")
    pre = importlib.import_module("neural-waveshaping-synthesis_amd.data.utils.preprocess_audio")
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
    audio = read_any(input_wav, sr, pre) if resample else read_mono(input_wav, sr)
    # frame-rate features, one frame per control hop: T = 1 + N // hop for both
    if stream_f0 is None:
        f0, voiced_prob = f0x.extract_f0_with_pyin(audio, sr, frame_length=1024, hop_length=hop, interpolate_fn=None)
    else:
        f0, voiced_prob = stream_f0_frames(audio, sr, hop, stream_f0, chunk)
    if stream_loudness is None:
        loudness = ldx.extract_perceptual_loudness(audio, sr, n_fft=1024, hop_length=hop, interpolate_fn=None)
    else:
        loudness = stream_loudness_frames(audio, hop, stream_loudness, chunk, loudness_reference, loudness_release, sr)
    f0 = f0 * 2.0 ** octave_shift
    f0_t, control = ck.make_control(f0, loudness, mean, std)
    if seed is not None:
        torch.manual_seed(seed)
    with torch.no_grad():
        out = model(f0_t.unsqueeze(0).cuda(), control.unsqueeze(0).cuda())
    y = out[0, :audio.size].cpu().numpy().astype(np.float32)
    if output_rate is not None and output_rate != sr:
        y, sr = pre.resample_audio(y, sr, output_rate), output_rate
    wavfile.write(output_wav, sr, y)
    print(f"{input_wav}: {audio.size} samples, {f0.size} frames, {100.0 * float(np.mean(voiced_prob > 0.5)):.0f} % voiced, "
          f"median F0 {float(np.median(f0)):.1f} Hz -> {output_wav}")


if __name__ == "__main__":
    main()
