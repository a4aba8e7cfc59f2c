"""Drop-in for the reference's process/make_test_data.py ("Test your own audio" of its README): one 16 kHz wav -> the test
side files GestureKNN.py takes, with the vq-wav2vec codes computed by qpgesture_amd/wavvq.py instead of fairseq.

    python -m qpgesture_amd.make_test_data --audio_path X.wav --save_path DIR --wavvq_model_path vq-wav2vec.pt --gpu 0

Writes into DIR (created if absent), with the reference's names and keys:
  <name>_wav.npz      wav    (n,) f32              the whole clip
  wav_240.npz         wav    (M, 64000) f32        its whole 4 s windows (wavlm.window_bounds: the reference's arithmetic)
  wavvq_240.npz       wavvq  (M, 398, 2) int64     the codes, the file --test_wavvq takes
  testing_data.npz    wav as above, and body, mfcc, txt, aux, energy, pitch, volume, context, phase as (2, 2, 2) f64
                      placeholders.  The reference fills them with np.random.rand - nothing reads their values in the
                      wavvq modes -; here they are ZEROS, so that the file is the same on every run.
The input must be 16 kHz PCM (wavlm.read_wav_16k): the reference resamples with librosa, this tool refuses another rate,
like the package's other command lines.  --wavvq_model_path is additive (the reference hard-codes ./vq-wav2vec.pt)."""
import argparse
import os

import numpy as np

from .wavlm import read_wav_16k, window_bounds

N_FRAMES, FPS = 240, 60
PLACEHOLDERS = ("body", "mfcc", "txt", "aux", "energy", "pitch", "volume", "context", "phase")


def process_audio(wavvq_model_path, audio_path, save_path, gpu_num="0", batch=32, model=None):
    """process_audio of the reference (make_test_data.py:10-70), same positional arguments; `model` (additive): a loaded
    WavVQ, or anything with forward_idx((B, n) f32) -> (B, T, G) codes, instead of the checkpoint at wavvq_model_path.
    Returns {name: path} of the four files."""
    os.makedirs(save_path, exist_ok=True)
    wav = read_wav_16k(audio_path)
    print(wav.shape)
    stem = os.path.splitext(os.path.basename(audio_path))[0]
    paths = dict(wav=os.path.join(save_path, stem + "_wav.npz"),
                 windows=os.path.join(save_path, "wav_%d.npz" % N_FRAMES),
                 wavvq=os.path.join(save_path, "wavvq_%d.npz" % N_FRAMES),
                 testing_data=os.path.join(save_path, "testing_data.npz"))
    np.savez_compressed(paths["wav"], wav=wav)
    bounds = window_bounds(len(wav), N_FRAMES, FPS)
    if not bounds:
        raise ValueError("%s has %d samples: shorter than one window of %d frames (%d samples)"
                         % (audio_path, len(wav), N_FRAMES, N_FRAMES * 16000 // FPS))
    source_wav = np.stack([wav[a:b] for a, b in bounds]).astype(np.float32)
    print(source_wav.shape)
    np.savez_compressed(paths["windows"], wav=source_wav)
    if model is None:
        from .wavvq import load_wavvq
        model = load_wavvq(wavvq_model_path, device="cuda:%s" % gpu_num)
    result = []
    for j in range(0, len(source_wav), batch):
        idx = model.forward_idx(source_wav[j:j + batch])
        result.append(idx.cpu().numpy() if hasattr(idx, "cpu") else np.asarray(idx))
    wavvq = np.vstack(result).astype(np.int64)
    print(wavvq.shape)
    np.savez_compressed(paths["wavvq"], wavvq=wavvq)
    tmp = np.zeros((2, 2, 2))
    np.savez_compressed(paths["testing_data"], wav=source_wav, **{k: tmp for k in PLACEHOLDERS})
    return paths


def main(argv=None):
    p = argparse.ArgumentParser(description="make_test_data")
    p.add_argument("--audio_path", type=str, default="../data/Example3/4.wav")
    p.add_argument("--save_path", type=str, default="../data/Example3/4")
    p.add_argument("--gpu", type=str, default="0")
    p.add_argument("--wavvq_model_path", type=str, default="./vq-wav2vec.pt")      # additive
    p.add_argument("--batch", type=int, default=32)                                # additive
    args = p.parse_args(argv)
    return process_audio(args.wavvq_model_path, args.audio_path, args.save_path, args.gpu, batch=args.batch)


if __name__ == "__main__":
    main()
