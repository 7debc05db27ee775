# Robust mIoU of a checkpoint of cmd/run_seg.sh on VOC 2012 val (the reference: main_advtrain.py --eval_pgd): every batch attacked in
# image space by sign-PGD, then scored.  Run from cv_a-fan_amd/.  Without the data: add --synthetic 64 (random images of VOC's sizes).
GPU=0
CKPT=checkpoints/voc_EXP01_selayer_3_sdlayer_aspp_gamma_se0.01_gamma_sd0.4_advweight0.3MIX11/best_deeplabv3plus_resnet50_voc_os16.pth

python -u main_seg_rob.py --year 2012 --crop_val \
--model deeplabv3plus_resnet50 \
--gpu_id ${GPU} \
--steps_pgd 3 --eps_pgd 8 --gamma_pgd 2 --clip_pgd \
--eval_pgd ${CKPT}
