#!/usr/bin/env python
"""Play a score on a trained model on MI355X: notes -> the note player (streaming.NotePlayer) -> wav.

    python scripts/play_score.py score.csv out.wav --model-checkpoint ckpt [--model-gin FILE] [--normalisation-dir dir] [--use-fastnewt]
                                 [--voices 16] [--hop-frames 1] [--stereo] [--tail-seconds S] [--seed N]
                                 [--attack F] [--decay F] [--release F] [--drop-db DB] [--silence X] [--peak-lo X] [--peak-hi X]
                                 [--vibrato-rate HZ] [--vibrato-depth CENTS] [--vibrato-delay F] [--vibrato-ramp F]

score.csv: one note per row, `onset_s,duration_s,pitch,velocity` (pitch: MIDI note number, fractions allowed; velocity in (0, 1]);
`#` starts a comment, empty lines are skipped.  With --stereo a fifth column `pan` in [-1, 1] places the note (default 0, centre).
Onsets and ends are rounded to hop boundaries (128 --hop-frames samples; a note lasts at least one hop).  A note that finds every
voice taken is dropped and counted.  After the last voice has stopped the reverb rings for --tail-seconds (default: the length of
the model's impulse response).  Times F are control frames of 128 samples; loudness values X are in the feature's units,
(dB + 80) / 80; the defaults are NotePlayer's.  Normalisation statistics are found as scripts/timbre_transfer.py finds them; the
wav is written as it writes its own (float32 at the model's rate).  Standard MIDI files are not read.  --model-gin FILE: a model of
another architecture (parsed on top of the packaged gin; the player then runs on the runtime-size slot stream), with
the weights of --model-checkpoint, or seeded random ones when none is named."""
import importlib
import math
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


def read_score(path):
    """-> [(onset_s, duration_s, pitch, velocity, pan), ...] in file order"""
    notes = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            row = [c.strip() for c in line.split("#", 1)[0].split(",")]
            if row == [""]:
                continue
            if len(row) not in (4, 5):
                raise click.BadParameter(f"{path}:{n}: expected onset_s,duration_s,pitch,velocity[,pan], got {line.strip()!r}")
            try:
                onset, duration, pitch, velocity = (float(c) for c in row[:4])
                pan = float(row[4]) if len(row) == 5 else 0.0
            except ValueError:
                raise click.BadParameter(f"{path}:{n}: not a number in {line.strip()!r}")
            if onset < 0 or duration <= 0 or not 0 < velocity <= 1 or not -1 <= pan <= 1:
                raise click.BadParameter(f"{path}:{n}: onset >= 0, duration > 0, velocity in (0, 1], pan in [-1, 1]")
            notes.append((onset, duration, pitch, velocity, pan))
    return notes


def hop_events(notes, hop_samples, sample_rate):
    """-> {hop: ([note index, ...] that start, [note index, ...] that end)}: onsets and ends rounded to hop boundaries"""
    events = {}
    for i, (onset, duration, _, _, _) in enumerate(notes):
        on = int(round(onset * sample_rate / hop_samples))
        off = max(on + 1, int(round((onset + duration) * sample_rate / hop_samples)))
        events.setdefault(on, ([], []))[0].append(i)
        events.setdefault(off, ([], []))[1].append(i)
    return events


def play(player, notes, sample_rate, tail_seconds):
    """the score through `player`, hop by hop -> (channels, samples) float32 on the CPU, and the number of dropped notes"""
    hop_samples = 128 * player.K
    events = hop_events(notes, hop_samples, sample_rate)
    last = max(events) if events else 0
    handles, out, hop = {}, [], 0
    while hop <= last or player.active() or player.stream.idle_slots() != list(range(player.B)):
        on, off = events.get(hop, ([], []))
        for i in on:
            handles[i] = player.note_on(notes[i][2], notes[i][3], notes[i][4])
        for i in off:
            player.note_off(handles.get(i))
        out.append(player.hop().cpu())
        hop += 1
    for _ in range(int(math.ceil(tail_seconds * sample_rate / hop_samples))):
        out.append(player.hop().cpu())
    return torch.cat(out, dim=1).numpy(), player.dropped


@click.command()
@click.argument("score_csv", type=click.Path(exists=True))
@click.argument("output_wav", type=click.Path())
@click.option("--model-gin", default=None, help="the model's gin file when it is not the packaged one (parsed on top of it)")
@click.option("--model-checkpoint", default=None, help="default: the packaged weights, or seeded random ones with --model-gin")
@click.option("--normalisation-dir", default=None, help="directory of data_mean.npy / data_std.npy (default: the checkpoint's)")
@click.option("--use-fastnewt", is_flag=True)
@click.option("--voices", default=16, type=click.IntRange(1, 65535), show_default=True, help="notes that can sound at once")
@click.option("--hop-frames", default=1, type=click.IntRange(1, 16), show_default=True, help="control frames per hop")
@click.option("--stereo", is_flag=True, help="two channels, notes placed by the score's fifth column (constant-power pan)")
@click.option("--tail-seconds", default=None, type=click.FloatRange(0.0), help="reverb tail after the last stop (default: the impulse response's length)")
@click.option("--seed", default=None, type=int, help="seed torch's generators, so that two runs draw the same start phases and noise")
@click.option("--attack", default=None, type=click.IntRange(0), help="attack, frames")
@click.option("--decay", default=None, type=click.IntRange(0), help="decay, frames")
@click.option("--release", default=None, type=click.IntRange(1), help="release, frames")
@click.option("--drop-db", default=None, type=click.FloatRange(0.0), help="sustain level below the peak, dB")
@click.option("--silence", default=None, type=float, help="loudness of silence, feature units")
@click.option("--peak-lo", default=None, type=float, help="peak loudness at velocity -> 0, feature units")
@click.option("--peak-hi", default=None, type=float, help="peak loudness at velocity 1, feature units")
@click.option("--vibrato-rate", default=None, type=click.FloatRange(0.0), help="Hz")
@click.option("--vibrato-depth", default=None, type=float, help="cents")
@click.option("--vibrato-delay", default=None, type=click.IntRange(0), help="frames before the vibrato fades in")
@click.option("--vibrato-ramp", default=None, type=click.IntRange(1), help="frames of the fade-in")
def main(score_csv, output_wav, model_gin, model_checkpoint, normalisation_dir, use_fastnewt, voices, hop_frames, stereo, tail_seconds,
         seed, attack, decay, release, drop_db, silence, peak_lo, peak_hi, vibrato_rate, vibrato_depth, vibrato_delay, vibrato_ramp):
    nws = importlib.import_module("neural-waveshaping-synthesis_amd")
    ck = importlib.import_module("neural-waveshaping-synthesis_amd.checkpoint")
    packaged = os.path.join(ROOT, "tests", "golden", "weights_vn.npz")
    nws.ensure_default_config()
    if model_gin:
        nws.gin.parse_config_file(model_gin)
    if model_checkpoint is None and model_gin:
        # another architecture without trained weights: what the player does and costs depends on the sizes, not on the values
        torch.manual_seed(0 if seed is None else seed)
        model = nws.NeuralWaveshaping().eval()
    else:
        model = nws.NeuralWaveshaping.load_from_checkpoint(model_checkpoint or packaged).eval()
    model_checkpoint = model_checkpoint or packaged             # where the normalisation statistics are looked for
    if use_fastnewt:
        model.newt = nws.FastNEWT(model.newt)
    model = model.cuda()
    sr = int(model.sample_rate)
    notes = read_score(score_csv)
    options = {"attack": attack, "decay": decay, "release": release, "drop": None if drop_db is None else drop_db / 80.0,
               "silence": silence, "peak_lo": peak_lo, "peak_hi": peak_hi, "vib_rate": vibrato_rate, "vib_depth": vibrato_depth,
               "vib_delay": vibrato_delay, "vib_ramp": vibrato_ramp}
    if seed is not None:
        torch.manual_seed(seed)
    with torch.no_grad():
        player = model.player(voices, hop_frames=hop_frames, channels=2 if stereo else 1,
                              normalisation=normalisation(ck, model_checkpoint, normalisation_dir),
                              **{k: v for k, v in options.items() if v is not None})
        if tail_seconds is None:
            tail_seconds = player.stream.tail_len / float(sr)
        y, dropped = play(player, notes, sr, tail_seconds)
        player.close()
    wavfile.write(output_wav, sr, np.ascontiguousarray(y.T if stereo else y[0], dtype=np.float32))
    print(f"{score_csv}: {len(notes)} notes ({dropped} dropped: every voice taken), {voices} voices, hops of {128 * hop_frames} samples -> "
          f"{output_wav}: {y.shape[1]} samples ({y.shape[1] / sr:.2f} s), {y.shape[0]} channel{'s' if stereo else ''}")


if __name__ == "__main__":
    main()
