"""Drop-in for step 3 of the reference's process/make_beat_dataset.py (:261-385, :604-607): encode every
240-frame pose window of a speaker database to 30 gesture codes (dataset_to_code) and, with --WavLM_model_path, every
4 s audio window to its WavLM features (wav_to_wavlm) - the two halves of the reference's step 3.

    python -m qpgesture_amd.make_beat_dataset --config codebook.yml --save_dir ../dataset/BEAT \
        --prefix speaker_10_state_0 --gpu 0 --step 3 --VQVAE_model_path codebook_checkpoint_best.bin \
        --WavLM_model_path WavLM-Large.pt

Reads  <save_dir>/<prefix>/<prefix>_<split>_240.npz['body'] (N,240,135) for split in train/validation/test,
writes <save_dir>/<prefix>/<prefix>_<split>_240_code.npz['code'] int64 (N,30) — the files GestureKNN.py takes
as --train_codebook.  With --WavLM_model_path ({'cfg', 'model'} checkpoint) it also reads the same files' ['wav']
(N,64000) and writes <prefix>_<split>_240_WavLM.npz['wavlm'] f32 (N,199,D), the --train_wavlm files, through the HIP
WavLM of qpgesture_amd/wavlm.py; with --WavVQ_model_path (a vq-wav2vec checkpoint, qpgesture_amd/wavvq.py) it writes
<prefix>_<split>_240_WavVQ.npz['wavvq'] int64 (N,398,2), the --train_wavvq files (wav_to_vq of the reference, :388-429);
without the flags nothing else changes.  Same flags as codebook/configs/parse_args.py.
The sentence embeddings of step 4 (make_txt_dataset's `context` column) are qpgesture_amd/sentence.py (txt_to_context,
`python -m qpgesture_amd.sentence`).  `--step 2` is the motion half of the reference's step 2:
<save_dir>/Motion/*.bvh of the speaker -> <prefix>/Rotation/*.npz and Rotation_20fps/*.npz, then the windowed
<prefix>_<split>_240.npz files where <prefix>/Wav exists (qpgesture_amd/process_bvh.py); step 1 (file copying) and the
audio, MFCC and transcript halves of step 2 are out of scope.

The reference encodes one window per call in a Python loop (:314-316); windows are independent, so they are
encoded in batches of 256 on the GPU (qpg_vq_encode_f32)."""
import argparse
import os

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(description='Codebook')
    p.add_argument('--config', default='./configs/codebook.yml')
    p.add_argument('--gpu', type=str, default='0')
    p.add_argument('--no_cuda', type=list, default=['0'])
    p.add_argument('--prefix', type=str, required=False, default='speaker_10_state_0')
    p.add_argument('--save_path', type=str, required=False, default="./Speech2GestureMatching/output/")
    p.add_argument('--code_path', type=str, required=False)
    p.add_argument('--VQVAE_model_path', type=str, required=False)
    p.add_argument('--BEAT_path', type=str, default="../dataset/orig_BEAT/speakers/")
    p.add_argument('--save_dir', type=str, default="../dataset/BEAT")
    p.add_argument('--step', type=str, default="3")
    p.add_argument('--stage', type=str, default="train")
    p.add_argument('--batch', type=int, default=256)       # additive
    p.add_argument('--WavLM_model_path', type=str, required=False)     # additive: also run wav_to_wavlm
    p.add_argument('--WavVQ_model_path', type=str, required=False)     # additive: also run wav_to_vq
    return p


def dataset_to_code(save_dir, prefix, n_frames=240, model_path=None, config=None, gpu="0", batch=256,
                    splits=("train", "validation", "test")):
    """dataset_to_code(save_dir, prefix, n_frames, model_path) of the reference (:261), same positional
    arguments; `config` = loaded codebook.yml (VQVAE hparams + data_mean/std)."""
    from .checkpoint import load_checkpoint, load_config
    from .vqvae import VQVAE, dataset_to_code as encode_windows
    if config is None:
        config = load_config(os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs", "codebook.yml"))
    model = VQVAE(config.VQVAE, 15 * 9, device="cuda:%s" % gpu)
    model.load_state_dict(load_checkpoint(model_path)["model_dict"])
    written = {}
    for key in splits:
        src = os.path.join(save_dir, prefix, prefix + '_' + key + '_' + str(n_frames) + '.npz')
        if not os.path.exists(src):
            continue
        poses = np.load(src)['body']                                       # (N, 240, 135)   (:292)
        print(poses.shape)
        code = encode_windows(model, poses.reshape(-1, n_frames, poses.shape[-1]), config.data_mean,
                              config.data_std, batch=batch)                # normalise (:296-301) + encode (:316)
        dst = os.path.join(save_dir, prefix, prefix + '_' + key + '_' + str(n_frames) + '_code' + '.npz')
        np.savez_compressed(dst, code=code)                                # (:321-322)
        written[key] = dst
    return written


def main(argv=None):
    from .checkpoint import load_config
    args = build_parser().parse_args(argv)
    if args.step == "2":
        from .process_bvh import process_speaker
        return process_speaker(args.save_dir, args.prefix, gpu=args.gpu)
    if args.step != "3":
        raise SystemExit("only --step 2 (BVH -> Rotation/, make_dataset: qpgesture_amd/process_bvh.py) and --step 3 "
                         "(dataset_to_code, wav_to_wavlm, wav_to_vq) are implemented; step 1 (file copying) is out of scope, "
                         "step 4's sentence embeddings are `python -m qpgesture_amd.sentence`")
    written = dataset_to_code(args.save_dir, args.prefix, 240, args.VQVAE_model_path, load_config(args.config),
                              gpu=args.gpu, batch=args.batch)
    if args.WavLM_model_path:
        from .wavlm import wav_to_wavlm
        wav_to_wavlm(args.save_dir, args.prefix, args.WavLM_model_path, gpu=args.gpu)
    if args.WavVQ_model_path:
        from .wavvq import wav_to_vq
        wav_to_vq(args.save_dir, args.prefix, args.WavVQ_model_path, gpu=args.gpu)
    return written


if __name__ == "__main__":
    main()
