# Same command line as the reference's Classification/cmd/run_base.sh (ResNet-56s baseline, no perturbation).
# Run from cv_a-fan_amd/ like the reference runs from Classification/.  Data parallel on one 8xMI355X node:
#   python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 main_base.py <same flags>
python -u main_base.py --seed 3 --save_dir base_res56s
